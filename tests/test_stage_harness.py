"""The two pieces of tests/stage_gpu.py and tests/mask_bits.py that every stage's GPU test relies on to catch a fault, checked on the CPU:
the guard band behind the output arrays must report a byte written into it, and the mask layout must be the header's."""
import numpy as np
import pytest

import mask_bits

torch = pytest.importorskip("torch")


def test_padded_reports_a_write_behind_an_array():
    from stage_gpu import PAD, Padded
    buf = Padded(device="cpu", a=24, b=8)
    raw = buf.host()
    assert {k: v.size for k, v in raw.items()} == {"a": 24, "b": 8} and all((v == 255).all() for v in raw.values())
    assert buf.a.numel() == 24 + PAD and buf.b.numel() == 8 + PAD and buf.pads_untouched()
    assert buf.view("a", np.uint32, (2, 3)).shape == (2, 3) and (buf.view("b", np.int64) == -1).all()
    buf.a[23] = 0                            # the last payload byte is the kernel's to write
    buf.host()
    assert buf.pads_untouched() and buf.raw["a"][23] == 0
    for name, at in (("a", 24), ("b", 8 + PAD - 1)):          # the first byte behind a, the last pad byte of b
        bad = Padded(device="cpu", a=24, b=8)
        getattr(bad, name)[at] = 0
        bad.host()
        assert not bad.pads_untouched(), (name, at)
        assert (bad.raw["a"] == 255).all() and (bad.raw["b"] == 255).all()


def test_mask_layout_and_round_trip():
    det = np.random.default_rng(3).random((3, 512)) < 0.5
    words = mask_bits.pack_mask(det)
    assert words.dtype == np.uint32 and words.shape == (3, 16)
    assert (mask_bits.unpack_mask(words, 512) == det).all()
    assert (mask_bits.unpack_mask(words.view(np.int32), 512) == det).all()          # the int32 tensors the tests hand over
    row = np.zeros((1, 512), bool)
    row[0, 33] = True
    assert mask_bits.pack_mask(row)[0].tolist() == [0, 2] + [0] * 14
    row[0, [0, 31, 511]] = True
    assert mask_bits.pack_mask(row)[0].tolist() == [0x80000001, 2] + [0] * 13 + [0x80000000]
