"""The head_dim-64 LSE / fp32 entries of band attention without a GPU (include/svg_attn_band_lse_d64.h): one validation table of the four
entries — every row is rejected on the host before any launch, the placeholder pointers are never read — and what the wrappers refuse."""
import ctypes as C

import pytest
import torch

from oracle import svg_oracle as O
from svg import _native as nat

BAD_ARG, UNSUPPORTED = -1, -2          # include/svg_attn.h
PH = 0x10000                           # placeholder device pointer (16-byte aligned)
NAMES = ("svg_band_attention_lse_d64", "svg_band_attention_lse_d64_f32", "svg_band_attention_switch_lse_d64",
         "svg_band_attention_switch_lse_d64_f32")


def _mask(S, **kw):
    m = nat.BandMask(S, 0, 0, 0, 0, 0)
    for key, val in kw.items():
        setattr(m, key, val)
    return m


def _args(name, q=PH, o=PH, lse=PH, BH=2, S=256, D=64, dtype=0, mask="ok", alt="ok", flag=PH):
    mask = _mask(S) if mask == "ok" else mask
    head = [q, PH, PH, o, lse, BH, S, D, dtype, 1.0, mask if mask is None else C.byref(mask), None]
    if "switch" in name:
        alt = _mask(S, band=S + 1) if alt == "ok" else alt
        head += [alt if alt is None else C.byref(alt), flag]
    return head + [None, None]


CASES = [
    ("null_lse", dict(lse=None), BAD_ARG),
    ("null_mask_D128", dict(mask=None, D=128), BAD_ARG),
    ("bad_band_D128", dict(mask=_mask(256, band=-1), D=128), BAD_ARG),
    ("D128", dict(D=128), UNSUPPORTED),
    ("dtype_f32", dict(dtype=2), UNSUPPORTED),
    ("o_8_bytes_off", dict(o=PH + 8, dtype=2), UNSUPPORTED),             # (o32 of the _f32 entries: unaligned; the others: the dtype)
    ("null_alt", dict(alt=None), BAD_ARG),
    ("null_flag_D128", dict(flag=None, D=128), BAD_ARG),
]


ROWS = [(name, cid, kw, code) for name in NAMES for cid, kw, code in CASES if "switch" in name or not {"alt", "flag"} & set(kw)]


@pytest.mark.parametrize("name,kw,expected", [(r[0], r[2], r[3]) for r in ROWS], ids=[f"{r[0]}-{r[1]}" for r in ROWS])
def test_validation_table(name, kw, expected):
    assert set(nat.BAND_LSE_D64_ENTRIES) == set(NAMES) and not set(NAMES) & set(nat.SIGNATURES)   # a table of their own
    assert getattr(nat.load(), name)(*_args(name, **kw)) == expected


def test_existing_wrappers_still_refuse_head_dim_64_and_the_new_ones_everything_else(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda *a, **k: pytest.fail("refused before the library is loaded"))
    q64, q128 = (torch.zeros(1, 2, 64, D, dtype=torch.bfloat16) for D in (64, 128))
    mask, flag = nat.BandMask(**O.dense_band_params(64)), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="return_lse"):
        nat.band_attention(q64, q64, q64, mask, return_lse=True)
    with pytest.raises(ValueError, match="return_lse"):
        nat.band_attention_switch(q64, q64, q64, mask, mask, flag, return_lse=True)
    for call in (lambda x, **kw: nat.band_attention_lse_d64(x, x, x, mask, **kw),
                 lambda x, **kw: nat.band_attention_switch_lse_d64(x, x, x, mask, mask, flag, **kw)):
        with pytest.raises(ValueError, match="head_dim 64"):
            call(q128)


@pytest.mark.parametrize("switched", [False, True])
def test_core_takes_the_lse_launch_at_head_dim_64_only_where_the_request_asks(monkeypatch, switched):
    from svg.models import _core

    calls, logged = [], []
    for name, ret in (("band_attention", "o"), ("band_attention_lse_d64", ("o", "lse"))):
        for name in (name, name.replace("attention", "attention_switch")):
            monkeypatch.setattr(_core._native, name, lambda *a, _n=name, _r=ret, **kw: calls.append((_n, kw)) or _r, raising=False)
    monkeypatch.setattr(_core, "sample_mse", lambda *a, **kw: torch.zeros(2, 2, 3))
    monkeypatch.setattr(_core, "_switch_generator", lambda: None)
    monkeypatch.setattr(_core, "log_quality", lambda quality, o, lse, *a, **kw: logged.append((o, lse)))
    q = type("Cuda", (), dict(is_cuda=True, dtype=torch.bfloat16, shape=(2, 3, 512, 64)))()   # (a stand-in that says it is on the GPU)
    geo = _core.Geometry(128, 3, 128)
    m, dm, flag = nat.BandMask(421, 128, 384, 421, 384, 421), nat.BandMask(421, 513, 0, 0, 0, 0), torch.zeros(1, dtype=torch.int32)
    for ask, entry, lse in ((False, "band_attention", None), (True, "band_attention_lse_d64", "lse")):
        quality = _core.QualityRequest("q.jsonl")
        quality.kept_mass_d64 = ask
        if switched:
            out = _core.svg1_attention_device_switch(q, q, q, geo, m, dm, None, 8, 384, flag, quality=quality)
        else:
            out = _core.svg1_sparse_attention(q, q, q, geo, m, None, 8, 384, quality=quality)
        name, kw = calls.pop()
        assert name == entry.replace("attention", "attention_switch") if switched else name == entry
        assert len(out) == 2 and out[0] == "o" and logged.pop() == ("o", lse) and "return_lse" not in kw and not calls
