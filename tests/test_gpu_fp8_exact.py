"""Exact-arithmetic tests of the e4m3 attention path: the quantise / placement / V-transpose pre-pass alone (byte for byte), and both
bodies (attn_body_f8pp behind band_attention_fp8, attn_body_f8g behind varblock_attention(fp8=True)) on inputs for which every
intermediate is exactly representable (tests/fp8_exact_cases.py), against the float64 result rounded once.  No tolerance for e4m3 noise:
a key dropped at a band edge, a probability missing from l or O, a wrong alpha, a neighbour's 1 / sv, a non-zero pad row or one wrong V^T
slot all leave the bound, which tests/test_fp8_exact_cases_cpu.py shows the reference itself keeps."""
import pytest
import torch

import fp8_exact_cases as X

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _run_prepass(nat, q, k, v, flags):
    """stage 1 of svg_band_attention_fp8_stage into a pre-poisoned workspace -> (parsed CPU workspace, placement keywords)"""
    from poisoned import POISON_BYTE, poisoned

    BH, S = q.shape[0], q.shape[1]
    need = X.workspace_offsets(BH, S)["total"]
    assert int(nat.load().svg_band_attention_fp8_workspace_bytes(BH, S, X.D)) == need
    ws = poisoned(need, dtype=torch.uint8)
    assert ws.data_ptr() % 64 == 0          # the offsets of fp8_exact_cases assume it (the library aligns the amax pointer, not the offset)
    kw = {}
    if flags is not None:
        kw = dict(head_perm_flag=torch.tensor([list(flags)]).cuda(), vid0=X.PLACE["vid0"], num_frame=X.PLACE["F"], frame_size=X.PLACE["P"])
    mask = nat.BandMask(**X.BAND_MASKS["dense"])
    nat.band_attention_fp8(q.cuda()[None], k.cuda()[None], v.cuda()[None], mask, sm_scale=X.SM_SCALE, workspace=ws, stage=1, **kw)
    torch.cuda.synchronize()
    w = X.parse_workspace(ws.cpu(), BH, S)
    assert (w["tail"] == POISON_BYTE).all()                 # nothing is written behind the scales
    return w


def _check_words(w, ref, q, k, v):
    """amax and scales of the workspace: amax bit for bit, 2^e with its E8M0 word, 1 / sv, the fourth word 0, the head's largest |q8|"""
    amax = torch.stack([t.float().abs().amax(dim=(-2, -1)) for t in (q, k, v)], dim=1)
    assert torch.equal(w["amax_bits"], amax.view(torch.int32))
    s0 = w["scales"][:, 0].double()
    e = torch.log2(s0).round().long()
    assert torch.equal(torch.exp2(e.double()), s0)                                   # a power of two
    assert torch.equal(w["scale_bits"][:, 2].long(), (127 + e) * 0x01010101)
    assert (w["scale_bits"][:, 3] == 0).all()
    top = X.e4m3_decode(w["q8"]).abs().amax(dim=(-2, -1))
    zero_head = amax[:, 0] == 0
    assert ((top >= 224) & (top <= 448))[~zero_head].all() and (top[zero_head] == 0).all()
    assert torch.equal(e, ref["e"]), (e, ref["e"])
    inv_sv = w["scales"][:, 1].double()
    assert ((inv_sv - ref["scales"][:, 1]).abs() <= 2.0 ** -21 * ref["scales"][:, 1]).all()     # 1 / (448 / av): two fast-math divisions


@pytest.mark.parametrize("flags", [None, X.PLACE["flags"]], ids=["plain", "placement"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inputs", X.BAND_INPUTS)
def test_prepass_lossless_bit_exact(nat, inputs, dtype, flags):
    """(a) lossless inputs: the three images byte for byte (pad rows included), amax, scales"""
    c = X.band_case(inputs, "dense")
    q, k, v = (c[n].to(dtype) for n in "qkv")
    kw = dict(flags=flags, vid0=X.PLACE["vid0"], F=X.PLACE["F"], P=X.PLACE["P"]) if flags else {}
    ref = X.prepass_reference(q, k, v, X.BAND_S, scale_log2=X.SCALE_LOG2, **kw)
    w = _run_prepass(nat, q, k, v, flags)
    for img in ("q8", "k8", "vt8"):
        diff = w[img] != ref[img]
        assert not diff.any(), f"{img}: {int(diff.sum())} bytes differ, first at {diff.nonzero()[0].tolist()}"
    _check_words(w, ref, q, k, v)
    assert w["q8"].shape[1] == 640 and (w["q8"][:, X.BAND_S:] == 0).all() and (w["k8"][:, X.BAND_S:] == 0).all()


@pytest.mark.parametrize("flags", [None, X.PLACE["flags"]], ids=["plain", "placement"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", X.PREPASS_SEEDS)
def test_prepass_random_inputs(nat, seed, dtype, flags):
    """(b) randn inputs against the products x * s formed in float64: a byte may differ only where the product lies within 2^-18 of the
    midpoint of two adjacent e4m3 values (the scale comes from fast-math fp32 divisions), and is then the other neighbour; at most 1 % of
    the elements are excused that way; no byte is a NaN encoding"""
    q, k, v = X.random_prepass_inputs(seed, dtype)
    kw = dict(flags=flags, vid0=X.PLACE["vid0"], F=X.PLACE["F"], P=X.PLACE["P"]) if flags else {}
    ref = X.prepass_reference(q, k, v, X.BAND_S, **kw)
    w = _run_prepass(nat, q, k, v, flags)
    _check_words(w, ref, q, k, v)
    for img, prod in (("q8", "prod_q"), ("k8", "prod_k"), ("vt8", "prod_vt")):
        got, want, p = w[img], ref[img], ref[prod]
        assert not X.is_e4m3_nan(got).any(), f"{img}: NaN encodings"
        excusable = X.near_midpoint(p)
        share = float(excusable.double().mean())
        diff = got != want
        print(f"[fp8 exact] pre-pass seed {seed} {dtype} {'placement' if flags else 'plain'} {img}: {int(diff.sum())} of {diff.numel()} bytes "
              f"differ from the float64 reference, {100 * share:.4f} % of the elements lie within 2^-18 of a rounding midpoint")
        assert share <= 0.01
        bad = diff & ~excusable
        assert not bad.any(), f"{img}: {int(bad.sum())} bytes differ away from any rounding midpoint, first at {bad.nonzero()[0].tolist()}"
        lo, hi, _ = X.e4m3_neighbours(p)
        mag, sign = (got & 0x7F).long(), got >= 128
        assert (((mag == lo) | (mag == hi)) & (sign == torch.signbit(p)))[diff].all(), f"{img}: a differing byte is not one of the two neighbours"
        assert (got.view(-1)[(p == 0).view(-1)] & 0x7F == 0).all()
    assert (w["q8"][:, X.BAND_S:] == 0).all() and (w["k8"][:, X.BAND_S:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask_name", list(X.BAND_MASKS))
@pytest.mark.parametrize("inputs", X.BAND_INPUTS)
def test_band_body_exact(nat, inputs, mask_name, dtype):
    """(c) band_attention_fp8 on the lossless cases: every element is dtype(ref64) or adjacent to it (the final acc * (inv_v / l) is the only
    inexact operation), elements whose reference is 0 and rows without keys are exactly 0.  The placement case takes its reference as
    test_band_attention_fused_placement does: placement -> attention -> inverse placement."""
    c = X.band_case(inputs, mask_name)
    q, k, v = (c[n].to(dtype)[None].cuda() for n in "qkv")
    kw = {}
    if c["place"]:
        pl = c["place"]
        kw = dict(head_perm_flag=torch.tensor([list(pl["flags"])]).cuda(), vid0=pl["vid0"], num_frame=pl["F"], frame_size=pl["P"])
    o = nat.band_attention_fp8(q, k, v, nat.BandMask(**c["prm"]), sm_scale=X.SM_SCALE, **kw)
    torch.cuda.synchronize()
    X.assert_exact_or_adjacent(o[0].cpu(), c["ref"], dtype, f"band body {inputs} {mask_name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("permuted", [False, True], ids=["in_order", "row_idx"])
def test_gathering_body_exact(nat, permuted, dtype):
    """(d) varblock_attention(fp8=True): Hq 4, Hkv 2, S 357, 5 x 9 ragged blocks with 1-row blocks and block-rows without an active key
    block, q_row_idx / kv_row_idx permutations; element mask from the oracle's block_mask_to_element_mask; the bound of (c)"""
    c = X.varblock_case(permuted)
    q, k, v = (c[n].to(dtype).cuda() for n in "qkv")
    kw = dict(q_row_idx=c["q_idx"].cuda(), kv_row_idx=c["k_idx"].cuda()) if permuted else {}
    o = nat.varblock_attention(q, k, v, c["block_map"].cuda(), c["q_sizes"].cuda(), c["k_sizes"].cuda(), sm_scale=X.SM_SCALE, fp8=True, **kw)
    torch.cuda.synchronize()
    assert (~c["em"].any(-1)).any()                       # the case has rows without keys
    X.assert_exact_or_adjacent(o.cpu(), c["ref"], dtype, f"gathering body {'row_idx' if permuted else 'in order'}")
