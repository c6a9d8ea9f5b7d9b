"""Half-split RoPE (rope_kind 3: channel i rotates against i + D / 2, the diffusers `use_real_unbind_dim=-2` form Cosmos uses) in the
fused QK prologue kernels: svg_qk_norm_rope[_qscale] (in place) and svg_qk_norm_rope_transpose[_qscale] (token-major in, head-major out).

The statement the kernel is held to, bit for bit: the existing kernel with the same norm and rope_kind 0, then
svg.models.cosmos.attention.apply_rotary_emb_half on the rotated rows — computed by torch on CPU tensors, so that the reference does not
depend on the GPU build of torch.  Shapes: the smallest at which the kernel can still go wrong — Hq = 5 is no multiple of the head unroll
(4) and differs from Hkv = 3; S = 151 is odd and no multiple of the rows per wave (2 ... 16) at any D; rope_lo = 7 and rope_hi = 140 put
both range edges inside a wave's rows.  The tables hold independent random values in all D columns: cos[:, i] != cos[:, i + D / 2], which
is what catches a kernel that reads half a table, or its partner's entry."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BSZ, HQ, HKV, S, LO, HI = 2, 5, 3, 151, 7, 140
EPS = 1e-6
BAD = -1


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def make_case(D, dtype, norm_kind, seed=0):
    g = torch.Generator().manual_seed(1000 * D + 10 * norm_kind + seed)
    c = dict(D=D, dtype=dtype, norm_kind=norm_kind)
    c["q"] = torch.randn(BSZ, HQ, S, D, generator=g).to(dtype)
    c["k"] = torch.randn(BSZ, HKV, S, D, generator=g).to(dtype)
    w = lambda: (1 + 0.1 * torch.randn(D, generator=g)).to(dtype)  # noqa: E731
    b = lambda: (0.1 * torch.randn(D, generator=g)).to(dtype)      # noqa: E731
    c["qw"], c["kw"] = (w(), w()) if norm_kind else (None, None)
    c["qb"], c["kb"] = (b(), b()) if norm_kind == 2 else (None, None)
    c["cos"] = torch.randn(HI - LO, D, generator=g)   # independent values in every column (not cos / sin of duplicated angles)
    c["sin"] = torch.randn(HI - LO, D, generator=g)
    assert not torch.equal(c["cos"][:, :D // 2], c["cos"][:, D // 2:]) and not torch.equal(c["sin"][:, :D // 2], c["sin"][:, D // 2:])
    return c


def dev(t):
    return None if t is None else t.cuda()


def norm_only(nat, c, which="qk"):
    """the existing kernel: same norm, rope_kind 0 -> CPU tensors (q, k)"""
    q, k = c["q"].clone().cuda(), c["k"].clone().cuda()
    if "q" in which:
        nat.qk_norm_rope(q, None, c["norm_kind"], dev(c["qw"]), dev(c["qb"]), None, None, EPS, 0)
    if "k" in which:
        nat.qk_norm_rope(k, None, c["norm_kind"], dev(c["kw"]), dev(c["kb"]), None, None, EPS, 0)
    return q.cpu(), k.cpu()


def rotate_cpu(x, cos, sin, lo=LO, hi=HI):
    from svg.models.cosmos.attention import apply_rotary_emb_half

    assert not x.is_cuda and not cos.is_cuda
    out = x.clone()
    out[:, :, lo:hi] = apply_rotary_emb_half(x[:, :, lo:hi], (cos, sin))
    return out


def run_inplace(nat, c, q=True, k=True, q_scale=1.0, lo=LO, hi=HI, kind=3):
    qq, kk = c["q"].clone().cuda(), c["k"].clone().cuda()
    a = (c["norm_kind"], dev(c["qw"]), dev(c["qb"]), dev(c["kw"]), dev(c["kb"]), EPS, kind, dev(c["cos"]), dev(c["sin"]), lo, hi)
    if q and k:
        nat.qk_norm_rope(qq, kk, *a, q_scale=q_scale)
    elif q:
        nat.qk_norm_rope(qq, None, a[0], a[1], a[2], None, None, *a[5:], q_scale=q_scale)
    else:   # k alone: it travels in the q slot of the wrapper (q_scale 1) ...
        nat.qk_norm_rope(kk, None, a[0], a[3], a[4], None, None, *a[5:])
    return qq.cpu(), kk.cpu()


def tok(x):
    """head-major [bsz, H, S, D] -> the token-major projection layout [bsz, S, H * D]"""
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1).contiguous()


def run_transpose(nat, c, q_scale=1.0):
    return tuple(t.cpu() for t in nat.qk_norm_rope_transpose(
        tok(c["q"]).cuda(), tok(c["k"]).cuda(), HQ, HKV, c["norm_kind"], dev(c["qw"]), dev(c["qb"]), dev(c["kw"]), dev(c["kb"]), EPS, 3,
        dev(c["cos"]), dev(c["sin"]), LO, HI, q_scale=q_scale))


@pytest.mark.parametrize("norm_kind", [0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_half_split_equals_norm_then_torch_rotation(nat, D, dtype, norm_kind):
    c = make_case(D, dtype, norm_kind)
    qn, kn = norm_only(nat, c)
    want_q, want_k = rotate_cpu(qn, c["cos"], c["sin"]), rotate_cpu(kn, c["cos"], c["sin"])
    got_q, got_k = run_inplace(nat, c)
    assert torch.equal(got_q, want_q) and torch.equal(got_k, want_k)
    assert not torch.equal(got_q, qn)                      # (the rotation did something)
    # the transposing entry on the token-major input equals the in-place entry on the head-major copy
    tq, tk = run_transpose(nat, c)
    assert tq.shape == got_q.shape and tk.shape == got_k.shape
    assert torch.equal(tq, got_q) and torch.equal(tk, got_k)


@pytest.mark.parametrize("D", [32, 128])
def test_q_only_and_k_only(nat, D):
    c = make_case(D, torch.bfloat16, 1, seed=1)
    qn, kn = norm_only(nat, c)
    got_q, untouched_k = run_inplace(nat, c, q=True, k=False)
    assert torch.equal(got_q, rotate_cpu(qn, c["cos"], c["sin"])) and torch.equal(untouched_k, c["k"])
    untouched_q, got_k = run_inplace(nat, c, q=False, k=True)
    assert torch.equal(got_k, rotate_cpu(kn, c["cos"], c["sin"])) and torch.equal(untouched_q, c["q"])
    # ... and through the NULL-q form of the C entry point itself (k in the k slot)
    lib = nat.load()
    kk, kw, cs, sn = c["k"].clone().cuda(), c["kw"].cuda(), c["cos"].cuda(), c["sin"].cuda()
    rc = lib.svg_qk_norm_rope_qscale(None, kk.data_ptr(), BSZ, 0, HKV, S, D, 0, 1, None, None, kw.data_ptr(), None, EPS, 3, cs.data_ptr(),
                                     sn.data_ptr(), LO, HI, 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(kk.cpu(), got_k)
    # the transposing entry, q alone
    tq, none = nat.qk_norm_rope_transpose(tok(c["q"]).cuda(), None, HQ, 0, 1, c["qw"].cuda(), None, None, None, EPS, 3, cs, sn, LO, HI)
    assert none is None and torch.equal(tq.cpu(), got_q)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_q_scale_single_rounding(nat, dtype):
    """q_scale multiplies the fp32 rotation in front of the ONE rounding (the half-split counterpart of
    tests/test_gpu_prescaled.py::test_prologue_q_scale_single_rounding); k does not see it."""
    D = 128
    c = make_case(D, dtype, 1, seed=2)
    scale = nat.softmax_q_scale(D)
    assert abs(scale - math.log2(math.e) / math.sqrt(D)) < 1e-6
    q1, k1 = run_inplace(nat, c)
    qc, kc = run_inplace(nat, c, q_scale=scale)
    assert torch.equal(kc, k1)
    qn, _ = norm_only(nat, c, "q")
    x = qn[:, :, LO:HI]
    x_real, x_imag = x.reshape(*x.shape[:-1], 2, -1).unbind(-2)
    x_rot = torch.cat([-x_imag, x_real], dim=-1)
    fp32 = x.float() * c["cos"][None, None] + x_rot.float() * c["sin"][None, None]
    assert torch.equal(fp32.to(dtype), q1[:, :, LO:HI])
    assert torch.equal(qc[:, :, LO:HI], (fp32 * scale).to(dtype))
    assert torch.equal(qc[:, :, :LO], (qn[:, :, :LO].float() * scale).to(dtype))
    assert torch.equal(qc[:, :, HI:], (qn[:, :, HI:].float() * scale).to(dtype))
    tq, tk = run_transpose(nat, c, q_scale=scale)
    assert torch.equal(tq, qc) and torch.equal(tk, kc)


@pytest.mark.parametrize("D", [32, 256])
def test_empty_position_range_is_rope_kind_0(nat, D):
    c = make_case(D, torch.float16, 2, seed=3)
    qn, kn = norm_only(nat, c)
    lib = nat.load()
    q, k = c["q"].clone().cuda(), c["k"].clone().cuda()
    t = {n: c[n].cuda() for n in ("qw", "qb", "kw", "kb", "cos", "sin")}
    rc = lib.svg_qk_norm_rope(q.data_ptr(), k.data_ptr(), BSZ, HQ, HKV, S, D, 1, 2, t["qw"].data_ptr(), t["qb"].data_ptr(),
                              t["kw"].data_ptr(), t["kb"].data_ptr(), EPS, 3, t["cos"].data_ptr(), t["sin"].data_ptr(), LO, LO,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(q.cpu(), qn) and torch.equal(k.cpu(), kn)


def test_rejections(nat):
    """kind 4 on the four extended entries, kind 3 on the entry that normalises across heads: SVG_ERR_BAD_ARG, before any launch"""
    lib = nat.load()
    D = 64
    q = torch.zeros(1, 2, 16, D, dtype=torch.bfloat16, device="cuda")
    o = torch.ones_like(q)
    tb = torch.zeros(16, D, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    qp, op, tp = q.data_ptr(), o.data_ptr(), tb.data_ptr()
    for kind, want in ((4, BAD), (-1, BAD), (3, 0)):
        assert lib.svg_qk_norm_rope(qp, None, 1, 2, 0, 16, D, 0, 0, None, None, None, None, EPS, kind, tp, tp, 0, 16, st) == want
        assert lib.svg_qk_norm_rope_qscale(qp, None, 1, 2, 0, 16, D, 0, 0, None, None, None, None, EPS, kind, tp, tp, 0, 16, 1.0, st) == want
        assert lib.svg_qk_norm_rope_transpose(qp, None, op, None, 1, 2, 0, 16, D, 0, 0, None, None, None, None, EPS, kind, tp, tp, 0, 16,
                                              st) == want
        assert lib.svg_qk_norm_rope_transpose_qscale(qp, None, op, None, 1, 2, 0, 16, D, 0, 0, None, None, None, None, EPS, kind, tp, tp, 0,
                                                     16, 1.0, st) == want
    assert lib.svg_rmsnorm_rope_transpose(qp, None, None, op, None, None, 1, 2, 16, D, 0, None, None, 0, EPS, 3, tp, tp, 0, 16, 1.0, st) == BAD
    torch.cuda.synchronize()
    assert torch.equal(q.cpu(), torch.zeros(1, 2, 16, D, dtype=torch.bfloat16))   # (zeros rotate to zeros: the kind-3 calls were harmless)
