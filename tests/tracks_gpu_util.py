"""The device buffers and the launch that test_tracks_gpu.py and test_tracks_carry_gpu.py share: the two arrays crn_segments_device
writes (the input of both track stages), the outputs of crn_tracks_device, and one call of it.  A plain module, not collected."""
import numpy as np
import torch

import crnsense as cs
from stage_gpu import DEV

# (slack_bins, max_miss, min_epochs, max_tracks)
SOME = [(1, 0, 1, 64), (0, 1, 2, 64), (2, 3, 1, 1024), (40, 1, 5, 64), (2, 0, 2, 1)]


class Segs:
    """The two arrays crn_segments_device writes, on the device."""

    def __init__(self, E, S):
        self.E, self.S = E, S
        self.epochs = torch.full((E, 16), 255, dtype=torch.uint8, device=DEV)
        self.segments = torch.full((E, S, 32), 255, dtype=torch.uint8, device=DEV)

    @classmethod
    def from_masks(cls, s, mask_t, spec_t, merge_gap=0, min_width=1, S=16):
        self = cls(mask_t.shape[0], S)
        s.segments_device(mask_t.data_ptr(), spec_t.data_ptr(), self.E, self.epochs.data_ptr(), self.segments.data_ptr(),
                          merge_gap=merge_gap, min_width=min_width, max_segments=S)
        return self

    @classmethod
    def from_host(cls, ep, segs):
        """Upload hand-made lists (tracks_f64.make_lists) in the kernel's layout."""
        E, S = segs.shape
        self = cls(E, S)
        e = np.zeros(E, cs.SEGMENT_EPOCH_DTYPE)
        e["n_found"], e["n_stored"] = ep["n_found"], ep["n_stored"]
        g = np.zeros((E, S), cs.SEGMENT_DTYPE)
        for f in ("lo", "width", "power", "peak_power", "centroid"):
            g[f] = segs[f]
        self.epochs = torch.from_numpy(np.frombuffer(e.tobytes(), np.uint8).reshape(E, 16).copy()).to(DEV)
        self.segments = torch.from_numpy(np.frombuffer(g.tobytes(), np.uint8).reshape(E, S, 32).copy()).to(DEV)
        return self

    def host(self):
        torch.cuda.synchronize()
        return (np.frombuffer(self.epochs.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE),
                np.frombuffer(self.segments.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(self.E, self.S))


class Tracks:
    """The outputs of crn_tracks_device, 0xFF at first (d_track_of 0x7F bytes: 0xFF would read as the legitimate label -1), and a
    workspace of exactly the size the library asks for."""

    def __init__(self, E, S, n_streams, max_tracks, max_miss=0):
        self.shape = (E, S, n_streams, max_tracks)
        self.streams = torch.full((n_streams, 16), 255, dtype=torch.uint8, device=DEV)
        self.tracks = torch.full((n_streams, max_tracks, 64), 255, dtype=torch.uint8, device=DEV)
        self.track_of = torch.full((E, S, 4), 0x7F, dtype=torch.uint8, device=DEV)
        self.ws_bytes = cs.tracks_workspace_bytes(E, S, E // n_streams, max_miss, 1, max_tracks)
        self.ws = torch.full((self.ws_bytes,), 255, dtype=torch.uint8, device=DEV)

    def host(self):
        E, S, n_streams, mt = self.shape
        torch.cuda.synchronize()
        return (np.frombuffer(self.streams.cpu().numpy().tobytes(), cs.TRACK_STREAM_DTYPE),
                np.frombuffer(self.tracks.cpu().numpy().tobytes(), cs.TRACK_DTYPE).reshape(n_streams, mt),
                np.frombuffer(self.track_of.cpu().numpy().tobytes(), np.int32).reshape(E, S))


def tracks(s, segs, eps, slack=1, miss=0, mine=1, mt=64, out=None, labels=True):
    """One crn_tracks_device call on `segs` cut into streams of eps epochs; returns the Tracks it wrote."""
    E, S = segs.E, segs.S
    out = Tracks(E, S, E // eps, mt, miss) if out is None else out
    s.tracks_device(segs.epochs.data_ptr(), segs.segments.data_ptr(), E, out.streams.data_ptr(), out.tracks.data_ptr(), out.ws.data_ptr(),
                    out.ws_bytes, track_of_ptr=out.track_of.data_ptr() if labels else 0, max_segments=S, epochs_per_stream=eps,
                    slack_bins=slack, max_miss=miss, min_epochs=mine, max_tracks=mt)
    return out
