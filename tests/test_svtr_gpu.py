"""The SVTR fork's mixing blocks on the MI355X: csrc/svtr.hip through the C ABI against tests/svtr_refs.py in float64, the
autograd wrapper variants.neighborhood_attention_2d, and htrvt_amd.svtr's modules against tests/golden/svtr.npz (the fork's own
modules in float64).

Kernel gates are the project's for window attention (tests/test_swin_gpu.py), against the float64 reference over the same
(already rounded) inputs: forward max-abs < 2.5e-2 (bfloat16) / 2e-5 (float32); dqkv within 3e-2 / 1e-4 of the tensor's
largest magnitude, cosine > 0.9995 / 0.999999.  Every output buffer (out, lse, dqkv) carries one canary row behind it that
must stay untouched.  (These are gates on a whole tensor.  The per-element gates of the kernels, with guard bands on both sides
of every output, live in tests/test_window_edges_gpu.py.)  Module gates are the project's, relative to the largest reference magnitude per tensor: float32 outputs
1e-3, gradients 2e-3; bfloat16 5e-2 and 1e-1.  Every parameter gradient is compared element by element with
svtr_refs.case_grads over the modules' own state_dicts, which tests/test_svtr_cpu.py anchors to the fork at 1e-10; the output
and the input gradient also with the fixture itself.  Every comparison prints what it observed (`pytest -s`).

Measured on an MI355X, worst over all parametrised cases: forward max-abs 8.3e-3 (bfloat16) / 7.7e-7 (float32); lse 7.6e-7;
dqkv 4.5e-3 / 7.6e-7 of its maximum, cosine 0.999997 / 1.0.  Modules, every gradient element by element: float32 outputs
7.6e-7, gradients 1.9e-6; bfloat16 outputs 7.6e-3, gradients 9.3e-3 for a single module and 2.0e-2 for the chain
(b0.norm1.weight, behind the bfloat16 backward of four modules): a fifth of the gate, nothing near it.  The whole file runs in
under 4 s; the past-2-GiB case takes 0.3 s.

Per-launch times (tools/bench_svtr.py, B = 128, heads of 32, 7 x 11 box, bfloat16, median of 7 windows of 20 launches; share
of the launch's HBM floor, the tensors read once and written once at 6.3 TB/s; beside them the dense route, the fused
attention kernel with a [heads, N, N] bias): 16x128 map, 2 heads: forward 128 us (0.17) against 587 us dense, backward 311 us
(0.14) against 5163 us; 8x128, 4 heads: 114 us (0.19) against 301 us, 290 us (0.15) against 2692 us; 4x128, 8 heads: 136 us
(0.16) against 164 us, 338 us (0.13) against 1560 us.  DESIGN 4m says what bounds them.
"""
import os

import numpy as np
import pytest
import torch

import svtr_cases as C
import svtr_refs as R

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
SHAPES = pytest.mark.parametrize("shape", C.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
FWD_ABS = {BF: 2.5e-2, F32: 2e-5}
GRAD_REL = {BF: 3e-2, F32: 1e-4}
GRAD_COS = {BF: 0.9995, F32: 0.999999}
MOD_OUT = {BF: 5e-2, F32: 1e-3}
MOD_GRAD = {BF: 1e-1, F32: 2e-3}
CANARY = 7.0


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import lib
    from htrvt_amd.ops import dt, ptr, stream
    return lib, ptr, stream, dt


def _out(shape, dtype):
    """an output buffer of `shape` with one canary row (the last dimension) behind it -> (whole buffer, the output's view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + shape[-1],), CANARY, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


def _canary_ok(buf, shape):
    return bool((buf[int(np.prod(shape)):] == CANARY).all())


def _untouched(buf):
    return bool((buf == CANARY).all())


def run_kernel(shape, qkv, dout, dtype, backward=True, with_lse=True):
    """forward (and backward) through the C ABI with canaries -> (out, lse, dqkv), on the device"""
    lib, ptr, stream, dt = _lib()
    B, H, W, heads, hd, kh, kw = shape
    D, rows = heads * hd, B * H * W
    q = qkv.to(dtype).cuda().contiguous()
    obuf, out = _out((rows, D), dtype)
    lbuf, lse = _out((B * heads, H * W), F32)
    rc = lib.htrvt_attn_nbr2d_fwd(ptr(q), ptr(out), ptr(lse) if with_lse else None, B, H, W, heads, hd, kh, kw, hd ** -0.5,
                                  dt(dtype), stream())
    assert rc == 0, lib.htrvt_last_error().decode()
    torch.cuda.synchronize()
    assert _canary_ok(obuf, (rows, D)) and (_canary_ok(lbuf, (B * heads, H * W)) if with_lse else _untouched(lbuf))
    if not backward:
        return out, lse, None
    g = dout.to(dtype).cuda().contiguous()
    dbuf, dqkv = _out((rows, 3 * D), dtype)
    rc = lib.htrvt_attn_nbr2d_bwd(ptr(q), ptr(out), ptr(g), ptr(lse), ptr(dqkv), B, H, W, heads, hd, kh, kw, hd ** -0.5,
                                  dt(dtype), stream())
    assert rc == 0, lib.htrvt_last_error().decode()
    torch.cuda.synchronize()
    assert _canary_ok(dbuf, (rows, 3 * D)) and _canary_ok(obuf, (rows, D)) and _canary_ok(lbuf, (B * heads, H * W))
    return out, lse, dqkv


def grad_check(name, got, ref, dtype):
    got, ref = got.detach().double().cpu().flatten(), ref.double().flatten()
    err = float((got - ref).abs().max() / ref.abs().max())
    cos = float(torch.dot(got, ref) / (got.norm() * ref.norm()))
    print(f"{name}: error {err:.3e} of max (gate {GRAD_REL[dtype]:.0e}), cosine {cos:.8f} (gate {GRAD_COS[dtype]})")
    assert err <= GRAD_REL[dtype] and cos > GRAD_COS[dtype], name


_REFS = {}


def kernel_ref(shape, dtype):
    """(inputs rounded to dtype, float64 out / dqkv over them), computed once per (shape, dtype)"""
    if (shape, dtype) not in _REFS:
        B, H, W, heads, hd, kh, kw = shape
        qkv, dout = C.kernel_inputs(shape, dtype)
        _REFS[(shape, dtype)] = (qkv, dout) + R.nbr2d_grads(qkv.double(), dout.double(), B, H, W, heads, (kh, kw))
    return _REFS[(shape, dtype)]


# ====================================================================== the kernels through the C ABI
@SHAPES
@DTYPES
def test_kernels_against_float64(shape, dtype):
    B, H, W, heads, hd, kh, kw = shape
    qkv, dout, out_r, dqkv_r = kernel_ref(shape, dtype)
    out, lse, dqkv = run_kernel(shape, qkv, dout, dtype)
    err = float((out.double().cpu() - out_r).abs().max())
    print(f"forward max-abs {err:.3e} (gate {FWD_ABS[dtype]:.1e})")
    assert err < FWD_ABS[dtype]
    assert bool(torch.isfinite(lse).all())
    grad_check("dqkv", dqkv, dqkv_r, dtype)


@pytest.mark.parametrize("shape", [C.KERNEL_SHAPES[1], C.KERNEL_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
@DTYPES
def test_lse_is_the_rows_log_sum_exp(shape, dtype):
    B, H, W, heads, hd, kh, kw = shape
    qkv, dout, _, _ = kernel_ref(shape, dtype)
    _, lse, _ = run_kernel(shape, qkv, dout, dtype, backward=False)
    q, k, _ = [t.transpose(1, 2) for t in qkv.double().view(B, H * W, 3, heads, hd).unbind(2)]
    S = (q @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(~R.visible(H, W, (kh, kw)), float("-inf"))
    err = float((lse.double().cpu().view(B, heads, H * W) - S.logsumexp(-1)).abs().max())
    print(f"lse max-abs {err:.3e}")
    assert err < 1e-4                                # float32 accumulation of at most 77 terms of order 1, in both dtypes


@DTYPES
def test_forward_without_lse_is_the_forward_with_it(dtype):
    shape = C.KERNEL_SHAPES[3]
    qkv, dout = C.kernel_inputs(shape, dtype)
    a = run_kernel(shape, qkv, dout, dtype, backward=False)[0]
    b = run_kernel(shape, qkv, dout, dtype, backward=False, with_lse=False)[0]
    assert torch.equal(a, b)


@DTYPES
def test_images_do_not_see_each_other_and_far_tokens_do_not_count(dtype):
    """token (4, 20) of image 1 changes: the outputs notice inside its box only, the gradients inside twice the box (dk of a
    key comes from the queries of its box, whose softmax holds the changed token when their own box does)"""
    shape = (2, 9, 60, 3, 32, 3, 11)
    B, H, W, heads, hd, kh, kw = shape
    qkv, dout = C.kernel_inputs(shape, dtype)
    out, _, dqkv = run_kernel(shape, qkv, dout, dtype)
    y, x = 4, 20
    q2 = qkv.clone()
    q2[H * W + y * W + x] = torch.randn(qkv.shape[1], generator=torch.Generator().manual_seed(9)).to(dtype)
    out2, _, dqkv2 = run_kernel(shape, q2, dout, dtype)
    ys, xs = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)

    def far(reach):
        keep = torch.ones(B, H * W, dtype=torch.bool)
        keep[1] = ~(((ys - y).abs() <= reach * (kh // 2)) & ((xs - x).abs() <= reach * (kw // 2))).reshape(-1)
        return keep.reshape(-1).cuda()

    assert int((~far(2)).sum()) < H * W              # the map is larger than twice the box: some tokens are far
    assert torch.equal(out[far(1)], out2[far(1)]) and torch.equal(dqkv[far(2)], dqkv2[far(2)])
    assert not torch.equal(out[~far(1)], out2[~far(1)])


@DTYPES
def test_backward_twice_gives_the_same_bits(dtype):
    qkv, dout = C.kernel_inputs(C.FORK_SHAPE, dtype)
    a, b = run_kernel(C.FORK_SHAPE, qkv, dout, dtype), run_kernel(C.FORK_SHAPE, qkv, dout, dtype)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_operands_past_two_gib():
    """qkv of more than 2^31 elements (4.4 GB in bfloat16): the offsets are 64-bit.  The first and the last image must come
    out as they do alone, bit for bit (an image's arithmetic does not depend on the batch)"""
    from htrvt_amd import seq_ops
    B, H, W, heads, hd, kernel = 2740, 16, 128, 2, 64, (7, 11)
    D, N = heads * hd, H * W
    assert B * N * 3 * D > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(B * N, 3 * D, device="cuda", dtype=BF, generator=g)
    dout = torch.randn(B * N, D, device="cuda", dtype=BF, generator=g)
    out, lse = seq_ops.nbr2d_attention_fwd(qkv, B, H, W, heads, kernel)
    dqkv = seq_ops.nbr2d_attention_bwd(qkv, out, dout, lse, B, H, W, heads, kernel)
    for b in (0, B - 1):
        rows = slice(b * N, (b + 1) * N)
        o1, l1 = seq_ops.nbr2d_attention_fwd(qkv[rows], 1, H, W, heads, kernel)
        d1 = seq_ops.nbr2d_attention_bwd(qkv[rows], o1, dout[rows], l1, 1, H, W, heads, kernel)
        assert torch.equal(out[rows], o1) and torch.equal(lse[b * heads:(b + 1) * heads], l1) and torch.equal(dqkv[rows], d1)
        assert float(o1.float().abs().max()) > 0.1 and bool(torch.isfinite(d1.float()).all())


def test_refusals_launch_nothing():
    lib, ptr, stream, dt = _lib()
    good = dict(B=2, H=4, W=16, heads=2, hd=32, kh=7, kw=11, dtype=dt(BF))
    bad = [(dict(hd=16), "head dim"), (dict(hd=128), "head dim"), (dict(hd=48), "head dim"), (dict(kh=6), "box"),
           (dict(kw=10), "box"), (dict(kh=9), "box"), (dict(kw=13), "box"), (dict(kh=0), "box"), (dict(kw=-1), "box"),
           (dict(H=0), "H=0"), (dict(heads=0), "heads=0"), (dict(B=-1), "B=-1"), (dict(dtype=2), "dtype"), (dict(off=1), "aligned")]
    tokens = 256                                     # room for every geometry below, served or not
    qbuf = torch.full((tokens * 3 * 256,), CANARY, dtype=BF, device="cuda")
    for change, word in bad:
        a = {**good, **change}
        off = a.pop("off", 0)
        obuf = torch.full((tokens * 256,), CANARY, dtype=BF, device="cuda")
        lbuf = torch.full((tokens * 2,), CANARY, device="cuda")
        dbuf = torch.full((tokens * 3 * 256,), CANARY, dtype=BF, device="cuda")
        geo = (a["B"], a["H"], a["W"], a["heads"], a["hd"], a["kh"], a["kw"], 0.125, a["dtype"], stream())
        rc = lib.htrvt_attn_nbr2d_fwd(ptr(qbuf), ptr(obuf) + 2 * off, ptr(lbuf), *geo)
        assert rc != 0 and word in lib.htrvt_last_error().decode(), (change, lib.htrvt_last_error())
        rc = lib.htrvt_attn_nbr2d_bwd(ptr(qbuf), ptr(obuf), ptr(obuf), ptr(lbuf), ptr(dbuf) + 2 * off, *geo)
        assert rc != 0 and word in lib.htrvt_last_error().decode(), (change, lib.htrvt_last_error())
        torch.cuda.synchronize()
        assert _untouched(obuf) and _untouched(dbuf) and _untouched(lbuf), change
        if "off" not in change and not set(change) & {"B", "H", "heads"}:        # _supported agrees with the launches
            assert lib.htrvt_attn_nbr2d_supported(a["hd"], a["kh"], a["kw"], a["dtype"]) == 0
            assert word in lib.htrvt_last_error().decode()
    assert lib.htrvt_attn_nbr2d_fwd(None, ptr(obuf), ptr(lbuf), 2, 4, 16, 2, 32, 7, 11, 0.125, dt(BF), stream()) != 0
    assert "null" in lib.htrvt_last_error().decode()
    assert lib.htrvt_attn_nbr2d_bwd(ptr(qbuf), ptr(obuf), ptr(obuf), None, ptr(dbuf), 2, 4, 16, 2, 32, 7, 11, 0.125, dt(BF),
                                    stream()) != 0 and "null" in lib.htrvt_last_error().decode()
    # more workgroups than a grid holds: refused, not wrapped (no buffer of that size is touched)
    assert lib.htrvt_attn_nbr2d_fwd(ptr(qbuf), ptr(obuf), ptr(lbuf), 1 << 21, 4096, 16, 2, 32, 7, 11, 0.125, dt(BF), stream()) != 0
    assert "workgroups" in lib.htrvt_last_error().decode()
    assert lib.htrvt_attn_nbr2d_fwd(ptr(qbuf), ptr(obuf), ptr(lbuf), 0, 4, 16, 2, 32, 7, 11, 0.125, dt(BF), stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(obuf) and _untouched(lbuf)
    for (hd, kh, kw, dtype), ok in (((32, 7, 11, BF), 1), ((64, 7, 11, F32), 1), ((64, 1, 1, BF), 1), ((32, 3, 5, F32), 1),
                                    ((32, 5, 9, BF), 1), ((128, 7, 11, BF), 0), ((16, 3, 3, F32), 0), ((32, 7, 12, BF), 0),
                                    ((32, 8, 11, BF), 0), ((32, 7, 13, BF), 0)):
        assert lib.htrvt_attn_nbr2d_supported(hd, kh, kw, dt(dtype)) == ok


# ====================================================================== the operator
@pytest.mark.parametrize("shape", [C.KERNEL_SHAPES[3], C.KERNEL_SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
@DTYPES
def test_operator_against_float64_autograd(shape, dtype):
    from htrvt_amd import variants
    B, H, W, heads, hd, kh, kw = shape
    qkv, dout, out_r, dqkv_r = kernel_ref(shape, dtype)
    assert variants.nbr2d_supported(hd, (kh, kw), dtype) and not variants.nbr2d_supported(hd, (kh, 12), dtype)
    q = qkv.cuda().requires_grad_(True)
    out = variants.neighborhood_attention_2d(q, B, H, W, heads, (kh, kw))
    (out.float() * dout.cuda().float()).sum().backward()
    err = float((out.detach().double().cpu() - out_r).abs().max())
    print(f"operator forward max-abs {err:.3e}")
    assert err < FWD_ABS[dtype]
    grad_check("dqkv", q.grad, dqkv_r, dtype)
    with pytest.raises(ValueError):
        variants.neighborhood_attention_2d(q, B, H, W, heads, (kh, 12))
    with pytest.raises(ValueError, match="qkv"):    # shapes that disagree with the geometry never reach the kernel
        variants.neighborhood_attention_2d(q, B + 1, H, W, heads, (kh, kw))
    with pytest.raises(ValueError, match="qkv"):
        variants.neighborhood_attention_2d(q[:, :-8], B, H, W, heads, (kh, kw))
    with pytest.raises(RuntimeError):
        variants.neighborhood_attention_2d(qkv, B, H, W, heads, (kh, kw))


# ====================================================================== the modules against the fork's goldens
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "svtr.npz"))


def rel(got, ref):
    ref = torch.as_tensor(ref, dtype=F64)
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def run_modules(mods, x, H, W):
    for _, kind, _, m in mods:
        if kind == "merge":
            x, H, W = m(x, H, W)
        else:
            x = m(x, H, W)
            H = 1 if kind == "comb" else H
    return x


def nodes_between(y):
    """names of the autograd nodes from y back to the leaves, along the one input of each that is no leaf"""
    names, fn = [], y.grad_fn
    while fn is not None:
        names.append(type(fn).__name__)
        nxt = [f for f, _ in fn.next_functions if f is not None and type(f).__name__ != "AccumulateGrad"]
        assert len(nxt) <= 1
        fn = nxt[0] if nxt else None
    return names


def check_modules(tag, mods, x, dy, H, W, dtype, gold_y=None, gold_dx=None):
    """forward and backward of the chain `mods` on the device against svtr_refs over the modules' own state_dicts"""
    for _, _, _, m in mods:
        m.cuda().eval()                              # Combining's drop = 0 aside, no module has train-only state
    xr = x.cuda().requires_grad_(True)
    y = run_modules(mods, xr, H, W)
    assert y.dtype == F32
    assert nodes_between(y) == ["_FunctionBackward"] * len(mods)         # one node per block / merging / combining
    (y * dy.cuda()).sum().backward()
    sds = [(t, kind, args, {k: v.detach().cpu() for k, v in m.state_dict().items()}) for t, kind, args, m in mods]
    y_ref, dx_ref, g_ref = R.case_grads(sds, x, dy, H, W)
    worst_out, worst, where = rel(y, y_ref), rel(xr.grad, dx_ref), "dx"
    if gold_y is not None:
        assert rel(y_ref, gold_y) < 1e-6 and rel(dx_ref, gold_dx) < 1e-6
        worst_out, worst = max(worst_out, rel(y, gold_y)), max(worst, rel(xr.grad, gold_dx))
    failed = []
    for t, _, _, m in mods:
        for n, p in m.named_parameters():
            key = f"{t}.{n}"
            assert p.grad is not None and p.grad.dtype == F32 and p.grad.shape == p.shape, key
            e = rel(p.grad, g_ref[key])
            print(f"  {tag} {key} {tuple(p.shape)}: {e:.3e}")
            if not e < MOD_GRAD[dtype]:
                failed.append((key, e))
            worst, where = max((worst, where), (e, key))
    print(f"{tag} {dtype}: outputs {worst_out:.2e} (gate {MOD_OUT[dtype]:.0e}), gradients {worst:.2e} at {where} "
          f"(gate {MOD_GRAD[dtype]:.0e})")
    assert not failed, failed
    assert worst_out < MOD_OUT[dtype] and worst < MOD_GRAD[dtype]
    return xr, y


@pytest.mark.parametrize("case", list(C.CASES))
@DTYPES
def test_modules_against_the_fork(gold, case, dtype):
    from htrvt_amd import svtr
    B, H, W, _, stages = C.CASES[case]
    x, dy = C.inputs(case)
    mods = C.case_modules(svtr, case, compute_dtype=dtype)
    for tag, _, _, m in mods:                        # rebuilt from their seeds: the modules the fixture's numbers come from
        for k, v in m.state_dict().items():
            assert abs(float(v.double().sum()) - float(gold[f"{case}.sums.{tag}.{k}"])) <= C.SUM_TOL * v.numel(), (tag, k)
    xr, y = check_modules(case, mods, x, dy, H, W, dtype, gold[f"{case}.y"], gold[f"{case}.dx"])
    assert tuple(y.shape) == C.out_shape(case)

    grads = [xr.grad.clone()] + [p.grad.clone() for _, _, _, m in mods for p in m.parameters()]
    for m in [m for _, _, _, m in mods]:
        m.zero_grad(set_to_none=True)
    wide = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], device="cuda")
    wide[:, :, ::2] = x.cuda()
    xn = wide[:, :, ::2].requires_grad_(True)        # the same values, not contiguous
    assert not xn.is_contiguous()
    y2 = run_modules(mods, xn, H, W)
    assert torch.equal(y2, y)
    (y2 * dy.cuda()).sum().backward()
    again = [xn.grad] + [p.grad for _, _, _, m in mods for p in m.parameters()]
    for a, b in zip(grads, again):                   # reproducible, and the same bits for the strided input
        assert torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(run_modules(mods, x.cuda(), H, W), y)


@pytest.mark.parametrize("local", [True, False], ids=["local", "global"])
@DTYPES
def test_stand_alone_attention_module(local, dtype):
    """MultiHeadSelfAttention on its own, a 3 x 5 box / the whole map of 40 tokens: one node, against svtr_refs"""
    from htrvt_amd import svtr
    torch.manual_seed(C.INIT_SEED)
    args = (64, 2, local, (3, 5))
    m = C.perturb(svtr.MultiHeadSelfAttention(*args, compute_dtype=dtype))
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(2, 40, 64, generator=g), torch.randn(2, 40, 64, generator=g)
    check_modules("attn", [("a", "attn", args, m)], x, dy, 5, 8, dtype)
    with pytest.raises(ValueError):
        m(x.cuda(), 5, 9)
