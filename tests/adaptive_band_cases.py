"""What tests/test_adaptive_band_cpu.py and tests/test_gpu_adaptive_band.py share (include/svg_attn_adaptive_band.h).  Plain module, no GPU.

  * the controller law of svg_band_width_update, twice: law32 — numpy fp32, every product and sum rounded where the kernel rounds, so the
    band it gives is the band the kernel must write, exactly — and law64, the float64 statement of the header;
  * the inputs, band vectors and element masks of the per-head attention cases: the geometry of tests/sparse_lse_cases.py with 4 heads."""
import functools

import numpy as np
import torch

import sparse_lse_cases as SC
from oracle import svg_oracle as O

H = 4
F32 = np.float32


def law32(band, kept, target, gain_up, gain_down, dead, quantum, band_min, band_max, skip=False):
    """int64 [BH]: the bands after one step, in the kernel's arithmetic.  kept: the fp32 values the kernel wrote."""
    band = np.asarray(band, dtype=np.int64)
    kept = np.asarray(kept, dtype=F32)
    if skip:
        return band.copy()
    target, gain_up, gain_down, dead = F32(target), F32(gain_up), F32(gain_down), F32(dead)
    out = band.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(band.size):
            kp = kept[h]
            if not np.isfinite(kp):
                continue
            e = F32(target - kp)
            x = F32(0)
            if e > 0:
                x = F32(gain_up * e)
            elif e < -dead:
                x = F32(gain_down * F32(e + dead))
            x = min(max(x, F32(-65536)), F32(65536))
            n = int(np.rint(x))                                          # ties to even, as rintf under the default rounding mode
            out[h] = min(max(int(band[h]) + n * int(quantum), int(band_min)), int(band_max))
    return out


def law64(band, kept, target, gain_up, gain_down, dead, quantum, band_min, band_max, skip=False):
    """the header's statement in float64 (parameters as Python floats)"""
    band = np.asarray(band, dtype=np.int64)
    kept = np.asarray(kept, dtype=np.float64)
    if skip:
        return band.copy()
    with np.errstate(invalid="ignore"):
        e = target - kept
        x = np.where(e > 0, gain_up * e, np.where(e < -dead, gain_down * (e + dead), 0.0))
        n = np.rint(np.clip(x, -65536, 65536))
    new = np.clip(band + np.where(np.isfinite(kept), n, 0).astype(np.int64) * quantum, band_min, band_max)
    return np.where(np.isfinite(kept), new, band)


def clamp_band(b, S):
    return min(max(int(b), 1), S + 1)


@functools.lru_cache(maxsize=None)
def inputs(model, dtype, seed=5):
    """q, k, v [1, 4, S, 128] on the CPU"""
    S = SC.band_case(model)[0]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, H, S, SC.D, generator=g).to(dtype) for _ in range(3))


def band_sets(S):
    """the band vectors of the bit tests: the extremes with two ordinary widths, and a set that straddles a q-tile edge"""
    return {"wide": [1, 129, 300, S + 1], "edge": [255, 256, 257, 64]}


def element_mask(model, band):
    """the model's element mask [S, S] with its band replaced"""
    S, prm, _, _ = SC.band_case(model)
    return O.band_mask(S, **dict(prm, band=int(band)))


@functools.lru_cache(maxsize=None)
def reference(model, dtype, bands):
    """float64 (o [1, 4, S, D], lse [1, 4, S]) of inputs(model, dtype) with head h under the element mask of band bands[h] (no placement)"""
    q, k, v = inputs(model, dtype)
    parts = [SC.masked_attention_lse(q[:, h:h + 1], k[:, h:h + 1], v[:, h:h + 1], element_mask(model, b)) for h, b in enumerate(bands)]
    return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)
