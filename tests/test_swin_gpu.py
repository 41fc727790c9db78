"""The Swin fork's blocks on the MI355X: csrc/swin.hip through the C ABI against tests/swin_refs.py in float64, the autograd
wrapper variants.window_attention_2d, and htrvt_amd.swin's modules against tests/golden/swin.npz (the fork's own modules in
float64).

Kernel gates are the project's for window attention (tests/test_lgp_kernels_gpu.py), against the float64 reference over the
same (already rounded) inputs: forward max-abs < 2.5e-2 (bfloat16) / 2e-5 (float32); dqkv and dtable within 3e-2 / 1e-4 of
the tensor's largest magnitude, cosine > 0.9995 / 0.999999.  Every output buffer, dtable_partial included, carries one
canary row behind it that must stay untouched.  (These are gates on a whole tensor.  The per-element gates of the kernels, with
guard bands on both sides of every output, live in tests/test_window_edges_gpu.py.)  Module gates are the VAN modules', relative to the largest reference
magnitude per tensor: float32 outputs 1e-3, gradients 2e-3; bfloat16 5e-2 and 1e-1.  Every parameter
gradient is compared element by element with swin_refs.case_grads over the modules' own state_dicts, which
tests/test_swin_cpu.py anchors to the fork at 1e-10; the output and the input gradient also with the fixture itself.  Every comparison prints what it observed (`pytest -s`).

Measured on an MI355X, worst over all parametrised cases: forward max-abs 1.4e-2 (bfloat16) / 7.8e-7 (float32); dqkv
4.7e-3 / 4.8e-7 of its maximum, cosine 0.999997 / 1.0; dtable 3.5e-7 / 3.8e-7 (dS is formed in float32 from the rounded
inputs in both dtypes).  Modules, every gradient element by element: float32 outputs 1.4e-6, gradients 6.9e-6; bfloat16 outputs
2.2e-2, gradients 9.9e-3 for the single block and 9.7e-2 for the chain (b1.mlp.0.weight; every parameter of b1 lies at 8e-2
... 9.7e-2, behind the bfloat16 backward of five modules -- the float32 figure times 2^16 would be 0.45).

Per-launch times (tools/bench_swin.py, B = 128, 6 heads, bfloat16; share of the launch's HBM floor, the tensors read once
and written once at 6.3 TB/s), unshifted / shifted: 4x128 map, 4x8 windows, hd 32 forward 41.4 / 40.0 us (0.39 / 0.40),
backward 167 / 160 us (0.17 / 0.18); 2x128, 2x8, hd 64 forward 37.8 / 37.3 us (0.42 / 0.43), backward 152 / 151 us (0.19);
1x128, 1x8, hd 128 forward 47.1 / 48.1 us (0.34 / 0.33), backward 175 / 176 us (0.16).  DESIGN 4l says what bounds them.
"""
import os

import numpy as np
import pytest
import torch

import swin_cases as C
import swin_refs as R

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


def run_kernel(shape, qkv, table, dout, dtype, backward=True):
    """forward (and backward) through the C ABI with canaries -> (out, dqkv, dtable, partial rows), on the device"""
    lib, ptr, stream, dt = _lib()
    B, H, W, heads, hd, wh, ww, sh, sw = shape
    D, rows_tok, TE = heads * hd, B * H * W, (2 * wh - 1) * (2 * ww - 1) * heads
    q, t = qkv.to(dtype).cuda().contiguous(), table.float().cuda().contiguous()
    obuf, out = _out((rows_tok, D), dtype)
    rc = lib.htrvt_attn_win2d_fwd(ptr(q), ptr(t), ptr(out), B, H, W, heads, hd, wh, ww, sh, sw, hd ** -0.5, dt(dtype), stream())
    assert rc == 0, lib.htrvt_last_error().decode()
    torch.cuda.synchronize()
    assert _canary_ok(obuf, (rows_tok, D))
    if not backward:
        return out, None, None, None
    g = dout.to(dtype).cuda().contiguous()
    rows = lib.htrvt_attn_win2d_rows(B, H, W, heads, wh, ww)
    assert rows >= 1
    dbuf, dqkv = _out((rows_tok, 3 * D), dtype)
    pbuf, partial = _out((rows, TE), F32)
    rc = lib.htrvt_attn_win2d_bwd(ptr(q), ptr(t), ptr(g), ptr(dqkv), ptr(partial), B, H, W, heads, hd, wh, ww, sh, sw, hd ** -0.5,
                                  dt(dtype), stream())
    assert rc == 0, lib.htrvt_last_error().decode()
    dtable = torch.zeros_like(t)
    assert lib.htrvt_rowsum_f32(ptr(partial), rows, TE, ptr(dtable), stream()) == 0
    torch.cuda.synchronize()
    assert _canary_ok(dbuf, (rows_tok, 3 * D)) and _canary_ok(pbuf, (rows, TE))
    return out, dqkv, dtable, partial


def grad_check(name, got, ref, dtype):
    got, ref = got.detach().double().cpu().flatten(), ref.double().flatten()
    err = float((got - ref).abs().max() / ref.abs().max())
    cos = float(torch.dot(got, ref) / (got.norm() * ref.norm()))
    print(f"{name}: error {err:.3e} of max (gate {GRAD_REL[dtype]:.0e}), cosine {cos:.8f} (gate {GRAD_COS[dtype]})")
    assert err <= GRAD_REL[dtype] and cos > GRAD_COS[dtype], name


_REFS = {}


def kernel_ref(shape, dtype):
    """(inputs rounded to dtype, float64 out / dqkv / dtable over them), computed once per (shape, dtype)"""
    if (shape, dtype) not in _REFS:
        B, H, W, heads, hd, wh, ww, sh, sw = shape
        qkv, table, dout = C.kernel_inputs(shape, dtype)
        _REFS[(shape, dtype)] = (qkv, table, dout) + R.win2d_grads(qkv.double(), table.double(), dout.double(), B, H, W, heads,
                                                                   (wh, ww), (sh, sw))
    return _REFS[(shape, dtype)]


# ====================================================================== the kernels through the C ABI
@SHAPES
@DTYPES
def test_kernels_against_float64(shape, dtype):
    qkv, table, dout, out_r, dqkv_r, dtable_r = kernel_ref(shape, dtype)
    out, dqkv, dtable, _ = run_kernel(shape, qkv, table, dout, dtype)
    err = float((out.double().cpu() - out_r).abs().max())
    print(f"forward max-abs {err:.3e} (gate {FWD_ABS[dtype]:.1e})")
    assert err < FWD_ABS[dtype]
    grad_check("dqkv", dqkv, dqkv_r, dtype)
    grad_check("dtable", dtable, dtable_r, dtype)


def test_partial_rows_of_the_many_window_shape():
    """the last kernel shape has more (image, window) items than partial rows x waves: more than one partial row per
    table entry, and every wave walks several items"""
    lib = _lib()[0]
    B, H, W, heads, hd, wh, ww, sh, sw = C.KERNEL_SHAPES[-1]
    rows = lib.htrvt_attn_win2d_rows(B, H, W, heads, wh, ww)
    assert rows > 1 and B * (H // wh) * (W // ww) > 4 * rows
    assert lib.htrvt_attn_win2d_rows(1, 4, 8, 6, 4, 8) == 1
    assert lib.htrvt_attn_win2d_rows(2, 4, 128, 6, 4, 9) < 0 and b"windows" in lib.htrvt_last_error()


@DTYPES
def test_additive_mask_is_pinned(dtype):
    """q = 32 e0 in the first region, k = 32 e0 in the second: the masked raw score is 181, so after -100 the masked keys
    still carry nearly all the weight.  A -inf or skipped mask fails here and nowhere else."""
    shape = (1, 1, 8, 1, 32, 1, 8, 0, 4)
    qkv, table = R.pinned_mask_case()
    assert torch.equal(qkv.to(dtype).double(), qkv)
    ref = R.win2d_attention(qkv, table, 1, 1, 8, 1, (1, 8), (0, 4))
    S, _, _ = R.win2d_scores(qkv, table, 1, 1, 8, 1, (1, 8), (0, 4))
    _, reg = R.window_slots(1, 8, (1, 8), (0, 4))
    P = S.softmax(-1)[0, 0, 0]
    assert float(P[reg[0] == 0][:, reg[0] != 0].sum(-1).min()) > 0.99
    out = run_kernel(shape, qkv, table, None, dtype, backward=False)[0]
    err = float((out.double().cpu() - ref).abs().max())
    print(f"pinned mask: max-abs {err:.3e}")
    assert err < FWD_ABS[dtype]


@DTYPES
def test_windows_and_images_do_not_see_each_other(dtype):
    shape = (2, 8, 16, 2, 32, 4, 8, 2, 4)
    B, H, W, heads, hd, wh, ww, sh, sw = shape
    qkv, table, dout = C.kernel_inputs(shape, dtype)
    out, dqkv, _, _ = run_kernel(shape, qkv, table, dout, dtype)
    tok, _ = R.window_slots(H, W, (wh, ww), (sh, sw))
    rows = H * W + tok[2]                            # window 2 of image 1
    q2 = qkv.clone()
    q2[rows] = torch.randn(len(rows), qkv.shape[1], generator=torch.Generator().manual_seed(9)).to(dtype)
    out2, dqkv2, _, _ = run_kernel(shape, q2, table, dout, dtype)
    keep = torch.ones(B * H * W, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(out[keep.cuda()], out2[keep.cuda()]) and torch.equal(dqkv[keep.cuda()], dqkv2[keep.cuda()])
    assert not torch.equal(out[~keep.cuda()], out2[~keep.cuda()])


@DTYPES
def test_one_unshifted_window_is_plain_biased_attention(dtype):
    shape = (1, 4, 8, 2, 32, 4, 8, 0, 0)
    qkv, table, dout = C.kernel_inputs(shape, dtype)
    ref = R.win2d_attention(qkv.double(), table.double(), 1, 4, 8, 2, (4, 8), (0, 0), masked=False)
    q, k, v = [t.permute(1, 0, 2) for t in qkv.double().view(32, 3, 2, 32).unbind(1)]
    bias = table.double()[R.table_index((4, 8))].permute(2, 0, 1)
    plain = ((q @ k.transpose(-1, -2) * 32 ** -0.5 + bias).softmax(-1) @ v).permute(1, 0, 2).reshape(32, 64)
    assert float((plain - ref).abs().max()) < 1e-12
    out = run_kernel(shape, qkv, table, dout, dtype, backward=False)[0]
    assert float((out.double().cpu() - plain).abs().max()) < FWD_ABS[dtype]


@DTYPES
def test_backward_twice_gives_the_same_bits(dtype):
    qkv, table, dout = C.kernel_inputs(C.FORK_SHAPE, dtype)
    a, b = run_kernel(C.FORK_SHAPE, qkv, table, dout, dtype), run_kernel(C.FORK_SHAPE, qkv, table, dout, dtype)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals_launch_nothing():
    lib, ptr, stream, dt = _lib()
    good = dict(B=2, H=4, W=16, heads=2, hd=32, wh=4, ww=8, sh=2, sw=4, dtype=dt(BF))
    bad = [(dict(hd=48), "head dim"), (dict(hd=16), "head dim"), (dict(wh=5, H=5), "tokens"), (dict(wh=0), "tokens"),
           (dict(H=6), "windows"), (dict(W=20), "windows"), (dict(sh=4), "shift"), (dict(sw=8), "shift"), (dict(sh=-1), "shift"),
           (dict(dtype=2), "dtype"), (dict(off=1), "aligned")]
    tokens = 256                                     # room for every geometry below, served or not
    qbuf = torch.full((tokens * 192,), CANARY, dtype=BF, device="cuda")
    table = torch.zeros(7 * 15, 2, device="cuda")
    for change, word in bad:
        a = {**good, **change}
        off = a.pop("off", 0)
        obuf = torch.full((tokens * 64,), CANARY, dtype=BF, device="cuda")
        dbuf = torch.full((tokens * 192,), CANARY, dtype=BF, device="cuda")
        pbuf = torch.full((64, 210), CANARY, device="cuda")
        geo = (a["B"], a["H"], a["W"], a["heads"], a["hd"], a["wh"], a["ww"], a["sh"], a["sw"], 0.125, a["dtype"], stream())
        rc = lib.htrvt_attn_win2d_fwd(ptr(qbuf), ptr(table), ptr(obuf) + 2 * off, *geo)
        assert rc != 0 and word in lib.htrvt_last_error().decode(), (change, lib.htrvt_last_error())
        rc = lib.htrvt_attn_win2d_bwd(ptr(qbuf), ptr(table), ptr(obuf), ptr(dbuf) + 2 * off, ptr(pbuf), *geo)
        assert rc != 0 and word in lib.htrvt_last_error().decode(), (change, lib.htrvt_last_error())
        torch.cuda.synchronize()
        assert _untouched(obuf) and _untouched(dbuf) and _untouched(pbuf), change
    assert lib.htrvt_attn_win2d_fwd(ptr(qbuf), None, ptr(obuf), 2, 4, 16, 2, 32, 4, 8, 0, 0, 0.125, dt(BF), stream()) != 0
    assert "null" in lib.htrvt_last_error().decode()
    for (hd, wh, ww, dtype), ok in (((32, 4, 8, BF), 1), ((64, 2, 8, F32), 1), ((128, 1, 32, BF), 1), ((128, 5, 6, F32), 1),
                                    ((96, 4, 8, BF), 0), ((32, 3, 11, BF), 0), ((32, 0, 8, BF), 0)):
        assert lib.htrvt_attn_win2d_supported(hd, wh, ww, dt(dtype)) == ok


# ====================================================================== the operator
@pytest.mark.parametrize("shape", [C.KERNEL_SHAPES[2], C.KERNEL_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
@DTYPES
def test_operator_against_float64_autograd(shape, dtype):
    from htrvt_amd import variants
    B, H, W, heads, hd, wh, ww, sh, sw = shape
    qkv, table, dout, out_r, dqkv_r, dtable_r = kernel_ref(shape, dtype)
    assert variants.win2d_supported(hd, (wh, ww), dtype) and not variants.win2d_supported(hd, (wh, 40), dtype)
    q, t = qkv.cuda().requires_grad_(True), table.cuda().requires_grad_(True)
    out = variants.window_attention_2d(q, t, B, H, W, heads, (wh, ww), (sh, sw))
    (out.float() * dout.cuda().float()).sum().backward()
    assert float((out.detach().double().cpu() - out_r).abs().max()) < FWD_ABS[dtype]
    grad_check("dqkv", q.grad, dqkv_r, dtype)
    grad_check("dtable", t.grad, dtable_r, dtype)
    with pytest.raises(ValueError):
        variants.window_attention_2d(q, t, B, H, W, heads, (wh, 40), (sh, sw))
    with pytest.raises(ValueError, match="qkv"):    # shapes that disagree with the geometry never reach the kernel
        variants.window_attention_2d(q, t, B + 1, H, W, heads, (wh, ww), (sh, sw))
    with pytest.raises(ValueError, match="qkv"):
        variants.window_attention_2d(q[:, :-8], t, B, H, W, heads, (wh, ww), (sh, sw))
    with pytest.raises(ValueError, match="table"):
        variants.window_attention_2d(q, t[:-1], B, H, W, heads, (wh, ww), (sh, sw))
    with pytest.raises(ValueError, match="table"):
        variants.window_attention_2d(q, t[:, :-1], B, H, W, heads, (wh, ww), (sh, sw))
    with pytest.raises(RuntimeError):
        variants.window_attention_2d(qkv, table, B, H, W, heads, (wh, ww), (sh, sw))


# ====================================================================== the modules against the fork's goldens
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "swin.npz"))


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


@pytest.mark.parametrize("case", list(C.CASES))
@DTYPES
def test_modules_against_the_fork(gold, case, dtype):
    from htrvt_amd import swin
    B, H, W, _, stages = C.CASES[case]
    x, dy = torch.from_numpy(gold[f"{case}.x"]), torch.from_numpy(gold[f"{case}.dy"])
    mods = C.case_modules(swin, case, compute_dtype=dtype)
    for tag, _, _, m in mods:                        # rebuilt from their seeds: the modules the fixture's numbers come from
        for k, v in m.state_dict().items():
            assert abs(float(v.double().sum()) - float(gold[f"{case}.sums.{tag}.{k}"])) <= C.SUM_TOL * v.numel(), (tag, k)
        m.cuda().train()
    xr = x.cuda().requires_grad_(True)
    y = run_modules(mods, xr, H, W)
    assert y.dtype == F32 and tuple(y.shape) == C.out_shape(case)
    assert nodes_between(y) == ["_FunctionBackward"] * len(stages)       # one node per block / merging / combining
    (y * dy.cuda()).sum().backward()
    # every gradient element by element against swin_refs over the modules' own state_dicts (test_swin_cpu.py anchors
    # swin_refs to the fork at 1e-10); the output and the input gradient against the fork's own numbers as well
    sds = [(tag, kind, args, {k: v.detach().cpu() for k, v in m.state_dict().items()}) for tag, kind, args, m in mods]
    y_ref, dx_ref, g_ref = R.case_grads(sds, x, dy, H, W)
    assert rel(y_ref, gold[f"{case}.y"]) < 1e-6 and rel(dx_ref, gold[f"{case}.dx"]) < 1e-6
    worst_out = max(rel(y, gold[f"{case}.y"]), rel(y, y_ref))
    worst, where = max(rel(xr.grad, gold[f"{case}.dx"]), rel(xr.grad, dx_ref)), "dx"
    failed = []
    for tag, _, _, m in mods:
        for n, p in m.named_parameters():
            key = f"{tag}.{n}"
            assert p.grad is not None and p.grad.dtype == F32 and p.grad.shape == p.shape, key
            e = rel(p.grad, g_ref[key])
            print(f"  {case} {key} {tuple(p.shape)}: {e:.3e}")
            if not e < MOD_GRAD[dtype]:
                failed.append((key, e))
            worst, where = max((worst, where), (e, key))
    print(f"{case} {dtype}: outputs {worst_out:.2e} (gate {MOD_OUT[dtype]:.0e}), gradients {worst:.2e} at {where} "
          f"(gate {MOD_GRAD[dtype]:.0e})")
    assert not failed, failed
    assert worst_out < MOD_OUT[dtype] and worst < MOD_GRAD[dtype]

    grads = [xr.grad.clone()] + [p.grad.clone() for _, _, _, m in mods for p in m.parameters()]
    for m in [m for _, _, _, m in mods]:
        m.zero_grad(set_to_none=True)
        m.eval()                                     # no train-only state at drop = 0: eval equals train, bit for bit
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


@DTYPES
def test_window_attention_module(dtype):
    """WindowAttention2D on partitioned windows without a mask, against swin_refs over its own state_dict"""
    from htrvt_amd import swin
    torch.manual_seed(C.INIT_SEED)
    m = C.perturb(swin.WindowAttention2D(64, 2, (2, 8), compute_dtype=dtype))
    sd = {k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(6, 16, 64, generator=g), torch.randn(6, 16, 64, generator=g)
    xr = x.double().requires_grad_(True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    ref = R.window_attention({**sd, **leaves}, xr, 2, (2, 8))
    (ref * dy.double()).sum().backward()
    m.cuda()
    xd = x.cuda().requires_grad_(True)
    y = m(xd)
    (y * dy.cuda()).sum().backward()
    assert rel(y, ref.detach()) < MOD_OUT[dtype] and rel(xd.grad, xr.grad) < MOD_GRAD[dtype]
    for n, p in m.named_parameters():
        assert rel(p.grad, leaves[n].grad) < MOD_GRAD[dtype], n
    with pytest.raises(NotImplementedError):
        m(xd, attn_mask=torch.zeros(6, 16, 16, device="cuda"))
