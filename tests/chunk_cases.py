"""Kernel cases of the optimizer entries that share the chunk table (facl_adam_apply, facl_ema_apply, facl_grad_sqnorm,
facl_adamw_apply): tensor sizes on both sides of a chunk and of a float4, aligned and one element off a 16-byte boundary, every
tensor between guard bands.  Shared by test_gpu_key_encoder.py and test_gpu_optim_recipe.py."""
import ctypes

import torch

DEV = "cuda:0"
SIZES = (1, 3, 4, 2047, 2048, 2049, 4100)                  # both sides of a 2048-element chunk and of a float4
SENTINEL = 12345.0
GUARD = 8                                                  # floats; 32 bytes keep the data 16-byte aligned behind it
CHUNK = 2048


def _case(nt):
    """nt = 14: every size of SIZES aligned, then every size with all tensors one float off a 16-byte boundary (the scalar walk).
    nt = 64: small tensors of 1..16 and 2044..2052 elements, alternating alignment."""
    if nt == 14:
        return [(n, s) for s in (0, 1) for n in SIZES]
    small = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 2044, 2047, 2048, 2049, 2050, 2052]
    return [(small[i % 16], (i // 16) % 2) for i in range(64)]


def _banded(values, shift, dtype=torch.float32):
    """[GUARD + shift sentinels | values | GUARD sentinels] in one allocation; shift = 1 puts the data one element off a
    16-byte boundary (fp32: 4 bytes).  Returns (buffer, data view)."""
    n = values.numel()
    buf = torch.full((GUARD + shift + n + GUARD,), SENTINEL, device=DEV, dtype=dtype)
    data = buf[GUARD + shift:GUARD + shift + n]
    data.copy_(values)
    assert buf.data_ptr() % 16 == 0 and data.data_ptr() % 16 == (data.element_size() * shift) % 16
    return buf, data


def _bands_intact(buf, shift, n):
    lo, hi = GUARD + shift, GUARD + shift + n
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[hi:] == SENTINEL).all())


def _chunks(case):
    return sum((n + CHUNK - 1) // CHUNK for n, _ in case)


def _ptrs(views):
    return (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])


def _ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])
