"""Float64 statements shared by tests/test_adaptive_top_p_cpu.py and tests/test_gpu_adaptive_top_p.py: the controller law of
svg_top_p_update (include/svg_attn_adaptive_top_p.h) and the per-head oracle of the block map.  kept_mass, params32 and ulps32 live in
tests/kept_mass_cases.py (both controllers' tests share them) and are re-exported here."""
import numpy as np
import torch

from kept_mass_cases import kept_mass, params32, ulps32  # noqa: F401
from oracle import svg_oracle as O


def law(p, kept, target, gain_up=1.0, gain_down=0.25, band=0.02, p_min=0.1, p_max=1.0):
    """float64 [BH]: the thresholds after one step.  kept not finite: unchanged."""
    p, kept = np.asarray(p, dtype=np.float64), np.asarray(kept, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = target - kept
        step = np.where(e > 0, gain_up * e, np.where(e < -band, gain_down * (e + band), 0.0))
        new = np.clip(p + step, p_min, p_max)
    return np.where(np.isfinite(kept), new, p)


def per_head_map(qc, kc, q_sizes, k_sizes, p_heads, min_kc_ratio=0.0):
    """oracle.identify_dynamic_map(exact=True) with one p per head: a LOOP over heads with a Python-float p.  (A broadcast p TENSOR would
    promote the compare `cumsum > p` to fp32 and skip the rounding of p to the input dtype — test_adaptive_top_p_cpu.py keeps a case.)
    qc [B, H, QC, D], p_heads: B * H floats -> bool [B, H, QC, KC]"""
    B, H = qc.shape[:2]
    out = []
    for i in range(B * H):
        b, h = divmod(i, H)
        out.append(O.identify_dynamic_map(qc[b:b + 1, h:h + 1], kc[b:b + 1, h:h + 1], q_sizes[b:b + 1, h:h + 1], k_sizes[b:b + 1, h:h + 1],
                                          float(p_heads[i]), min_kc_ratio, exact=True)[0, 0])
    return torch.stack(out).reshape(B, H, *out[0].shape)
