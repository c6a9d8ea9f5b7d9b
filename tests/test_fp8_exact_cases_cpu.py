"""The exact-arithmetic cases of the e4m3 attention path (tests/fp8_exact_cases.py) on the CPU: the inputs are in the lossless regime, the
torch restatement of attn_body_f8pp reproduces the float64 reference rounded once bit for bit on every band case the GPU tests run —
except on the few elements per case whose reference lies within 2^-23 of a rounding midpoint of the 16-bit format, where rounding to fp32
first can end on the other neighbour — so the reference alone stays inside the bound those tests ask of the kernel; a restatement with a
wrong mask edge, a wrong alpha or a probability missing from l does not; and the pre-pass reference round-trips."""
import pytest
import torch

import fp8_exact_cases as X
from oracle import svg_oracle as O

BAND_CASES = [(i, m) for i in X.BAND_INPUTS for m in X.BAND_MASKS]


def test_e4m3_table_and_rounding():
    assert X.E4M3_VALUES[0] == 0 and X.E4M3_VALUES[126] == 448 and (X.E4M3_VALUES.diff() > 0).all()
    g = torch.Generator().manual_seed(0)
    y = torch.cat([torch.randn(20000, generator=g).double() * s for s in (1e-3, 0.05, 1.0, 30.0, 200.0)])
    y = y.clamp(-448, 448)
    assert torch.equal(X.e4m3_bytes(y), y.to(torch.float8_e4m3fn).view(torch.uint8))          # agrees with torch away from the double rounding
    mids = (X.E4M3_VALUES[:-1] + X.E4M3_VALUES[1:]) / 2
    b = X.e4m3_bytes(mids)
    assert (b % 2 == 0).all() and X.near_midpoint(mids).all() and not X.near_midpoint(X.E4M3_VALUES[1:]).any()
    assert X.e4m3_bytes(torch.tensor([500.0, -500.0, -0.0, 0.0], dtype=torch.float64)).tolist() == [126, 254, 128, 0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_round_once_and_ordered(dtype):
    g = torch.Generator().manual_seed(1)
    y = torch.randn(50000, generator=g).double() * torch.exp2(torch.randint(-20, 12, (50000,), generator=g).double())
    r = X.round_once(y, dtype)
    lo_hi = torch.stack([(X.ordered(r) + d) for d in (-1, 1)])
    # nearest: no neighbour of the result is closer to y
    def value(o):
        bits = torch.where(o >= 0, o, (-o) | 0x8000).to(torch.int16)
        return bits.view(dtype).double()
    err = (r.double() - y).abs()
    assert (err <= (value(lo_hi[0]) - y).abs()).all() and (err <= (value(lo_hi[1]) - y).abs()).all()
    # a tie goes to the even significand, where a conversion through float32 can go wrong
    one = torch.tensor([1.0], dtype=dtype)
    ulp = float(value(X.ordered(one) + 1) - 1.0)
    t = torch.tensor([1 + ulp / 2, 1 + 3 * ulp / 2, 1 + ulp / 2 + 2.0 ** -40], dtype=torch.float64)
    assert X.round_once(t, dtype).double().tolist() == [1.0, 1 + 2 * ulp, 1 + ulp]


def test_generator_holds_its_conditions():
    """every input set the GPU tests use; lossless_inputs asserts the regime itself (check_lossless)"""
    for kind in X.BAND_INPUTS:
        q, k, v = X.band_case(kind, "dense")["q"], X.band_case(kind, "dense")["k"], X.band_case(kind, "dense")["v"]
        X.check_lossless(q, k, v)
        sc = X.head_scales(q, k, v)
        assert len(set(sc["sv"].tolist())) >= 3 and len(set(sc["e"].tolist())) >= 2      # the heads do not share their scales
    c = X.varblock_case(True)
    X.check_lossless(c["q"], c["k"], c["v"])
    s = X.band_case("structured", "dense")
    assert (s["q"][2] == 0).all() and (s["v"][3] == 0).all()
    x = s["x"]
    j = torch.arange(X.BAND_S) // 64
    assert torch.equal(x[0, 5], j.clamp(max=12).double()) and torch.equal(x[1, 400], (12 - j).clamp(min=0).double())
    # and a generator that leaves the regime is caught
    q, k, v = (t.clone() for t in (s["q"], s["k"], s["v"]))
    k[0, 3, 0] += 1.0
    with pytest.raises(AssertionError):
        X.check_lossless(q, k, v)


@pytest.mark.parametrize("name", list(X.BAND_MASKS))
def test_interval_mask_is_the_documented_predicate(name):
    prm = X.BAND_MASKS[name]
    assert torch.equal(X.interval_mask(X.BAND_S, prm), O.band_mask(X.BAND_S, **prm))
    tiles = X.band_q_tiles(X.BAND_S, prm)
    rows = sorted(r for q0, q_end, _ in tiles for r in range(q0, q_end))
    assert rows == list(range(X.BAND_S))
    mask = X.interval_mask(X.BAND_S, prm)
    for q0, q_end, ks in tiles:                     # every allowed key of a q-tile lies in a tile the kernel visits, once
        assert len(set(ks)) == len(ks)
        need = mask[q0:q_end].any(0).nonzero().flatten() // 64 * 64
        assert set(need.tolist()) <= set(ks)


def test_band_shape_reaches_every_part():
    dense = X.band_q_tiles(X.BAND_S, X.BAND_MASKS["dense"])
    assert [(a, b) for a, b, _ in dense] == [(0, 256), (256, 512), (512, 613)] and all(len(ks) == 10 for _, _, ks in dense)
    assert 512 + 4 * 32 >= 613           # waves 4 .. 7 of the last q-tile are idle
    b70 = X.band_q_tiles(X.BAND_S, X.BAND_MASKS["band70"])
    assert any(X._classify(X.BAND_S, X.BAND_MASKS["band70"], q0, q_end, ks[0], w) == X.TILE_SKIP
               for q0, q_end, ks in b70 for w in range(8) if q0 + 32 * w < q_end)
    assert len(X.band_q_tiles(X.BAND_S, X.BAND_MASKS["full_ranges"])) == 4


@pytest.mark.parametrize("inputs,name", BAND_CASES)
def test_emulation_equals_reference_rounded_once(inputs, name):
    c = X.band_case(inputs, name)
    emu = X.emulate_f8pp(c["x"], c["v_logical"], X.BAND_S, c["prm"])
    if c["place"]:
        emu = X.unplace(emu, c["place"]["flags"], X.BAND_S, c["place"]["vid0"], c["place"]["F"], c["place"]["P"])
    for dtype in (torch.bfloat16, torch.float16):
        want = X.round_once(c["ref"], dtype)
        got = emu.to(dtype)
        differ = got.view(torch.int16) != want.view(torch.int16)
        # Bit for bit, except where two roundings cannot equal one: the restatement (like the kernel) rounds inv_v / l and acc * inv to fp32,
        # a relative error of at most 2 * 2^-24, before it rounds to 16 bits.  Where ref64 lies that close to a rounding midpoint of the
        # 16-bit format the fp32 value can fall on the midpoint or beyond it, and the second rounding then goes to the other neighbour.
        # Nowhere else: a differing element must lie within 2^-23 of a midpoint (a handful per case do), and is then adjacent.
        excusable = X.near_rounding_midpoint(c["ref"], dtype, 2.0 ** -23)
        assert not (differ & ~excusable).any(), f"{int((differ & ~excusable).sum())} elements differ away from any rounding midpoint"
        # (exact ties are structurally common for these rationals, a few in 10^4; they are excusable too: inv_v / l is inexact there as well)
        assert float(excusable.double().mean()) < 1e-3
        share = X.assert_exact_or_adjacent(got, c["ref"], dtype, f"emulation {inputs} {name}")
        assert share >= 1 - float(excusable.double().mean())
    no_keys = ~c["mask"].any(1)
    ref_l = X.ref64(c["x"], c["v_logical"], c["mask"])
    assert (ref_l[:, no_keys] == 0).all()
    if inputs == "structured":
        ref = c["ref"]
        assert (ref[3] == 0).all()                                                  # v = 0
        mean = torch.matmul(c["mask"].double(), c["v_logical"][2]) / c["mask"].sum(1, keepdim=True).clamp(min=1)
        if c["place"]:
            mean = X.unplace(mean[None].repeat(4, 1, 1), c["place"]["flags"], X.BAND_S, c["place"]["vid0"], c["place"]["F"], c["place"]["P"])[2]
        assert torch.allclose(ref[2], mean, rtol=1e-14, atol=0)                     # q = 0: the plain mean of the allowed v


@pytest.mark.parametrize("mutation", X.MUTATIONS)
@pytest.mark.parametrize("inputs,name", BAND_CASES)
def test_wrong_emulation_differs(inputs, name, mutation):
    """the same restatement with one deliberate error leaves the bound of the GPU tests on every case: the bound can tell"""
    c = X.band_case(inputs, name)
    emu = X.emulate_f8pp(c["x"], c["v_logical"], X.BAND_S, c["prm"], mutate=mutation)
    if c["place"]:
        emu = X.unplace(emu, c["place"]["flags"], X.BAND_S, c["place"]["vid0"], c["place"]["F"], c["place"]["P"])
    for dtype in (torch.bfloat16, torch.float16):
        with pytest.raises(AssertionError):
            X.assert_exact_or_adjacent(emu.to(dtype), c["ref"], dtype, f"{mutation} {inputs} {name}")


@pytest.mark.parametrize("flags", [None, X.PLACE["flags"]])
@pytest.mark.parametrize("inputs", X.BAND_INPUTS)
def test_prepass_reference_round_trips(inputs, flags):
    c = X.band_case(inputs, "dense")
    q, k, v = c["q"], c["k"], c["v"]
    kw = dict(flags=flags, vid0=X.PLACE["vid0"], F=X.PLACE["F"], P=X.PLACE["P"]) if flags else {}
    ref = X.prepass_reference(q, k, v, X.BAND_S, scale_log2=X.SCALE_LOG2, **kw)
    qd, kd, vd = X.prepass_dequantise(ref, X.BAND_S, **kw)
    assert torch.equal(qd, q) and torch.equal(kd, k) and torch.equal(vd, v)
    S_pad = X.workspace_offsets(X.BAND_BH, X.BAND_S)["S_pad"]
    assert S_pad == 640 and ref["q8"].shape == (4, 640, 128) and ref["vt8"].shape == (4, 10, 128, 64)
    assert (ref["q8"][:, X.BAND_S:] == 0).all() and (ref["k8"][:, X.BAND_S:] == 0).all()
    for img, prod in (("q8", "prod_q"), ("k8", "prod_k"), ("vt8", "prod_vt")):
        assert torch.equal(X.e4m3_decode(ref[img]), ref[prod]) and not X.is_e4m3_nan(ref[img]).any()
    # the byte-slot order, stated independently: position 32 g + 16 b + 4 j + i of V^T row d in tile t is key 32 b + 8 j + 4 g + i
    vl = X.place(v, flags, X.BAND_S, **{n: X.PLACE[n] for n in ("vid0", "F", "P")}) if flags else v
    for (h, t, d, g, b, j, i) in ((0, 0, 0, 0, 0, 0, 0), (1, 3, 77, 1, 0, 2, 3), (2, 8, 127, 0, 1, 3, 1), (3, 9, 5, 1, 1, 0, 2), (1, 9, 64, 1, 0, 1, 0)):
        key = 64 * t + 32 * b + 8 * j + 4 * g + i
        want = float(vl[h, key, d] * ref["sv"][h]) if key < X.BAND_S else 0.0
        assert float(X.e4m3_decode(ref["vt8"])[h, t, d, 32 * g + 16 * b + 4 * j + i]) == want
    # scales of the lossless heads: 2^e with the E8M0 word, largest |q8| in [224, 448] or 0
    top = X.e4m3_decode(ref["q8"]).abs().amax(dim=(-2, -1))
    assert (((top >= 224) & (top <= 448)) | (top == 0)).all()
    o = X.workspace_offsets(X.BAND_BH, X.BAND_S)
    assert o["amax"] % 64 == 0 and o["total"] == 3 * 4 * 640 * 128 + 4 * 28 + 256


@pytest.mark.parametrize("seed", [31, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_random_prepass_inputs_have_few_near_ties(seed, dtype):
    """the seeds of the GPU pre-pass test on randn inputs: at most 1 % of the elements lie within 2^-18 of a rounding midpoint (those
    are the only ones the GPU test excuses)"""
    q, k, v = X.random_prepass_inputs(seed, dtype)
    ref = X.prepass_reference(q, k, v, X.BAND_S)
    for prod in ("prod_q", "prod_k", "prod_vt"):
        share = float(X.near_midpoint(ref[prod]).double().mean())
        assert share <= 0.01, (prod, share)
