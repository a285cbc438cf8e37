"""The two users of the shared run extraction (csrc/crn_mask_runs.h: run_plan<B>, join_spanning) pinned to each other on the MI355X.

With guard = 0, min_age = 1, first = 1, epochs_per_stream = 1 and avg_epochs = 1 the free mask of crn_holes_device is the complement of
its input mask and Pbar is the row itself, so the holes of a mask m are the segments of ~m from crn_segments_device with merge_gap = 0,
the same min_width and max_segments = max_holes: the same n_found and n_stored and, per stored slot, the same lo, width and peak_bin and
the same bytes of power and peak_power.  (noise_mean and floor_mean meet only through the float64 twins and are left out.)  The counts
are also held to the circular runs of the mask counted on the host, so that two kernels wrong alike do not pass."""
import numpy as np
import pytest

import crnsense as cs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402
MAX_OUT = (4, 16)        # 4: fewer slots than some rows have runs


def _min_widths(B):
    return (1, 5, B, B + 3, 3 * B + 1)     # B + 3, 3 B + 1: no run inside one lane piece is wide enough


def _free_masks(n):
    """[rows][n] bool and what each row is: the runs that must come out are the runs of True."""
    B, rng = n // 64, np.random.default_rng(n)
    rows, names = [], []

    def row(name, *spans):
        f = np.zeros(n, bool)
        for lo, w in spans:
            f[np.arange(lo, lo + w) % n] = True
        rows.append(f)
        names.append(name)

    row("empty")
    row("full", (0, n))
    row("full but one bin", (5 * B + 1, n - 1))
    row("one run crossing the wrap", (n - 5, 12))
    row("three whole lanes, from mid-lane to mid-lane", (10 * B + B // 2, B - B // 2 + 3 * B + B // 2 - 1))
    row("whole lanes across the wrap", (61 * B + 3, 5 * B))
    for w in _min_widths(B):
        # exactly min_width and one less: inside a lane where it fits, over a lane edge, over the wrap
        row(f"widths {w} and {w - 1}", (3 * B + B - 2, w), (30 * B + 1, max(w - 1, 1)), (50 * B, w))
        row(f"width {w - 1} over the wrap, {w} inside", (n - 1, max(w - 1, 1)), (20 * B + 1, w))
        row(f"width {w} over the wrap, {w - 1} inside", (n - w + 1, w), (20 * B + 1, max(w - 1, 1)))
    row("more runs than slots", *[(k * 3 * B + 1, 5 + k % 3) for k in range(1, 20)])
    row("more runs than slots, one over the wrap", (n - 3, 9), *[(k * 3 * B + 1, 5 + k % 3) for k in range(1, 20)])
    for density in (0.5, 0.9, 0.98):
        rows.append(rng.random(n) < density)
        names.append(f"random, {density} free")
    return np.array(rows), names


def _runs(f):
    """The widths of the maximal circular runs of True in f (the full circle: one run of len(f))."""
    n = f.size
    if f.all():
        return [n]
    k = int(np.argmin(f))                                     # a False bin: no run crosses the cut in front of it
    g = np.roll(f, -k).astype(np.int8)
    edges = np.diff(np.concatenate(([0], g, [0])))
    return list(np.flatnonzero(edges == -1) - np.flatnonzero(edges == 1))


@pytest.mark.parametrize("n", [512, 4096])
def test_holes_of_a_mask_are_the_segments_of_its_complement(built, n):
    B = n // 64
    free, names = _free_masks(n)
    E = free.shape[0]
    P = np.random.default_rng(n + 1).gamma(10.0, 1e-4, (E, n)).astype(np.float32)
    assert (P > 0).all()
    spec_t = sgpu.upload_rows(P)
    blocked_t = sgpu.upload_mask(~free)     # what crn_holes_device reads
    free_t = sgpu.upload_mask(free)         # what crn_segments_device reads
    widths = [_runs(f) for f in free]
    s = cs.Sensor(cs.cfg_energy_scaled(n))
    stored = 0
    for mw in _min_widths(B):
        want_found = np.array([sum(w >= mw for w in ws) for ws in widths])
        for mo in MAX_OUT:
            seg_e = torch.full((E, 16), 255, dtype=torch.uint8, device=DEV)
            seg_s = torch.full((E, mo, 32), 255, dtype=torch.uint8, device=DEV)
            s.segments_device(free_t.data_ptr(), spec_t.data_ptr(), E, seg_e.data_ptr(), seg_s.data_ptr(), merge_gap=0, min_width=mw, max_segments=mo)
            q = dict(guard=0, min_age=1, min_width=mw, max_holes=mo, avg_epochs=1)
            age = torch.full((E, n), -1, dtype=torch.int32, device=DEV)
            hol_e = torch.full((E, 32), 255, dtype=torch.uint8, device=DEV)
            hol_s = torch.full((E, mo, 32), 255, dtype=torch.uint8, device=DEV)
            ws_bytes = cs.holes_workspace_bytes(E, 1, **q)
            ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=DEV)
            s.holes_device(blocked_t.data_ptr(), spec_t.data_ptr(), E, age.data_ptr(), hol_e.data_ptr(), ws.data_ptr(), ws_bytes,
                           cs.hole_params(1, first=True, **q), holes_ptr=hol_s.data_ptr())
            torch.cuda.synchronize()
            se = np.frombuffer(seg_e.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE)
            ss = np.frombuffer(seg_s.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(E, mo)
            he = np.frombuffer(hol_e.cpu().numpy().tobytes(), cs.HOLE_STREAM_DTYPE)
            hs = np.frombuffer(hol_s.cpu().numpy().tobytes(), cs.HOLE_DTYPE).reshape(E, mo)
            what = f"N={n} min_width={mw} max={mo}"
            for e in range(E):
                at = (what, names[e])
                assert se["n_found"][e] == want_found[e] and he["n_found"][e] == want_found[e], (at, se["n_found"][e], he["n_found"][e], want_found[e])
                assert se["n_stored"][e] == min(want_found[e], mo) and he["n_stored"][e] == se["n_stored"][e], at
                k = int(se["n_stored"][e])
                for f in ("lo", "width", "peak_bin"):
                    assert (ss[f][e, :k] == hs[f][e, :k]).all(), (at, f, ss[f][e, :k], hs[f][e, :k])
                for f in ("power", "peak_power"):
                    assert ss[f][e, :k].tobytes() == hs[f][e, :k].tobytes(), (at, f, ss[f][e, :k], hs[f][e, :k])
                if want_found[e] <= mo:
                    assert sorted(ss["width"][e, :k]) == sorted(w for w in widths[e] if w >= mw), at
                stored += k
    s.close()
    print(f"N={n}: {E} rows x {len(_min_widths(B))} min_width x {len(MAX_OUT)} slot counts, {stored} stored runs compared")
