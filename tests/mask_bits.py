"""The bin-mask layout every detection stage shares (include/crn_sense.h, crn_sense_run_device_cfar): one definition for the float64
twins, which re-export the two names, and for the GPU tests' uploads (tests/stage_gpu.py)."""
import numpy as np


def pack_mask(det):
    """[E][N] bool -> [E][N / 32] uint32, bit k % 32 of word k / 32 = bin k (the layout crn_sense_run_device_cfar writes)."""
    det = np.asarray(det, bool)
    E, n = det.shape
    bits = det.reshape(E, n // 32, 32).astype(np.uint64)
    return (bits << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_mask(words, n):
    """The inverse; the words may be the int32 tensors' arrays the tests hand over: they are reinterpreted, not converted."""
    words = np.asarray(words).view(np.uint32).reshape(-1, n // 32)
    return ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1, n)
