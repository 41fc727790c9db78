"""The convolutional forks' modules in TRAIN mode with the forks' rates on the MI355X: FeedForward, ConvModule (with
drop_path), ConformerBlock, SqueezeConformerBlock and SqueezeFormerEncoder of htrvt_amd.conformer at the shapes of
tests/golden/conformer_dropout.npz, float32 and bfloat16, against tests/conformer_dropout_refs.py in float64 run with the
masks rebuilt on the host from the seeds the module kept (`last_drop_seeds`).  tests/test_conformer_dropout_cpu.py ties
those refs to the forks' own train-mode modules at 1e-10.

Gates are those of tests/test_squeezeformer_gpu.py::test_module_reproduces_the_fork: relative to the tensor's maximum,
float32 1e-3 (outputs) / 2e-3 (gradients), bfloat16 5e-2 / 1e-1.  A wrong mask anywhere moves an output by its own size.
bfloat16 at 40 tokens takes the fused attention kernels and float32 the batched-GEMM route: both are judged against the
same host mask, so the same seeds give the same attention mask on both.

Measured on an MI355X (output / worst gradient, relative to the tensor's maximum):
  float32:  ffn 3.4e-7 / 4.2e-7, conv 9.4e-8 / 5.0e-7, cblock 3.1e-7 / 6.2e-7, sblock 3.1e-7 / 6.1e-7, encoder 3.4e-7 / 9.3e-7
  bfloat16: ffn 5.0e-3 / 6.1e-3, conv 2.4e-3 / 1.1e-2, cblock 7.5e-3 / 8.2e-3, sblock 7.2e-3 / 1.3e-2, encoder 8.9e-3 / 1.5e-2"""
import numpy as np
import pytest
import torch

import attn_dropout_refs as A
import conformer_dropout_refs as DR
import squeezeformer_cases as C

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
CDTS = pytest.mark.parametrize("cdt", [F32, BF], ids=["f32", "bf16"])
SEEDS = range(11, 41)


def _host_masks(case, seeds):
    """(masks, rates, the sample masks of the drop-path sites) in the form conformer_dropout_refs.run takes"""
    kind, args, kwargs, B, N = DR.CASES[case]
    D, seeds = args[0], seeds.cpu().numpy()
    if kind == "ffn":
        assert seeds.shape == (2,)
        return torch.from_numpy(DR.site_masks(seeds, B * N, D, N, kwargs["dropout"], 0.0)[0]).double(), kwargs["dropout"], []
    if kind == "conv":
        assert seeds.shape == (2,)
        e, s = DR.site_masks(seeds, B * N, D, N, kwargs["dropout"], kwargs["drop_path"])
        return (torch.from_numpy(e).double(), torch.from_numpy(s).double()), (kwargs["dropout"], kwargs["drop_path"]), [s]
    rates = DR.block_rates(case)
    if kind != "encoder":
        assert seeds.shape == (9,)
        m = DR.block_masks(seeds, rates, B, N, D, args[1])
        return m, rates, [s.numpy() for s in m["S"]]
    assert seeds.shape == (2, 9)
    ms = [DR.block_masks(seeds[0], rates[0], B, N, D, args[1]), DR.block_masks(seeds[1], rates[1], B, N // 2, D, args[1])]
    return ms, rates, [s.numpy() for s in ms[1]["S"]]           # the first block's drop-path rate is 0


def _mixed(paths):
    return all(0 < float(np.sum(s)) < len(s) for s in paths)


_PICKED, _REFS = {}, {}


def _seed_for(case, m, x):
    """the first seed of SEEDS at which every drop-path site of the case keeps a sample and drops one (a forward only)"""
    if case not in _PICKED:
        for seed in SEEDS:
            torch.cuda.manual_seed(seed)
            with torch.no_grad():
                m.train()(x)
            if _mixed(_host_masks(case, m.last_drop_seeds)[2]):
                break
        _PICKED[case] = seed
    return _PICKED[case]


def _reference(case, seeds):
    key = (case,) + tuple(seeds.cpu().reshape(-1).tolist())
    if key not in _REFS:
        from htrvt_amd import conformer
        kind, args = DR.CASES[case][:2]
        sd = {k: v.double() for k, v in DR.case_module(conformer, case).state_dict().items()}
        x, dy = [t.double() for t in DR.inputs(case)]
        masks, rates, _ = _host_masks(case, seeds)
        _REFS[key] = DR.module_grads(kind, args, sd, x, dy, C.NORM_EPS, masks, rates)
    return _REFS[key]


def _rel(name, got, ref, gate):
    ref = torch.as_tensor(ref, dtype=F64)
    err = float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max() / ref.abs().max())
    print(f"  {name}: {err:.2e} (gate {gate:.0e})")
    assert err < gate, (name, err)
    return err


@CDTS
@pytest.mark.parametrize("case", list(DR.CASES))
def test_module_trains_as_the_fork(case, cdt):
    """train-mode forward and backward with the forks' rates: one autograd node; two runs from the same
    torch.cuda.manual_seed agree bit for bit and another seed gives other masks; the seeds kept are pairwise distinct; some
    sample is dropped and some kept at every drop-path site; outputs and gradients are the float64 reference's with the masks
    rebuilt from those seeds; eval mode is the module with zero rates, bit for bit"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import conformer
    kind, args, kwargs, B, N = DR.CASES[case]
    go, gg = (1e-3, 2e-3) if cdt == F32 else (5e-2, 1e-1)
    x, dy = [t.cuda() for t in DR.inputs(case)]
    m = DR.case_module(conformer, case, compute_dtype=cdt).cuda()
    seed = _seed_for(case, m, x)
    print(f"\n{case} {cdt} seed {seed}")
    runs, kept = [], []
    for s in (seed, seed, seed + 100):
        torch.cuda.manual_seed(s)
        m.zero_grad()
        xr = x.clone().requires_grad_(True)
        y = m.train()(xr)
        assert y.grad_fn is not None and y.grad_fn.name().startswith("_Function")
        assert y.dtype == F32 and xr.grad is None
        y.backward(dy)
        runs.append([y.detach(), xr.grad] + [p.grad.clone() for p in m.parameters()])
        kept.append(m.last_drop_seeds.clone())
    assert kept[0].dtype == torch.int64 and kept[0].is_cuda
    assert torch.equal(kept[0], kept[1]) and not torch.equal(kept[0], kept[2])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], runs[2][0])
    flat = kept[0].reshape(-1).tolist()
    assert len(set(flat)) == len(flat)
    _, _, paths = _host_masks(case, kept[0])
    assert kind == "ffn" or (paths and _mixed(paths))

    y_r, dx_r, g_r = _reference(case, kept[0])
    worst = _rel("dx", runs[0][1], dx_r, gg)
    _rel("y", runs[0][0], y_r, go)
    for (n, p), g_ in zip(m.named_parameters(), runs[0][2:]):
        assert g_.dtype == F32 and g_.shape == p.shape
        worst = max(worst, _rel("grad " + n, g_, g_r[n], gg))
    print(f"  worst gradient error {worst:.2e}")

    zero = {k: 0.0 for k in kwargs if "drop" in k}
    m0 = C.case_module(conformer, (kind, args, dict(kwargs, **zero)), compute_dtype=cdt).cuda()
    with torch.no_grad():
        assert torch.equal(m.eval()(x), m0.eval()(x))
        assert torch.equal(m0.train()(x), m0.eval()(x))              # zero rates: train mode is eval mode
    assert m0.last_drop_seeds is None


@CDTS
def test_attention_routes_share_the_mask(cdt):
    """seq_ops.plain_attention_fwd / _bwd with drop=(seed, p) at 40 tokens: bfloat16 (the fused kernels) and float32 (the
    batched GEMMs) both match the float64 attention with the host mask of that seed, and miss it with another seed's"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import seq_ops
    B, N, h, hd, p = DR.B, DR.N, DR.HEADS, DR.D // DR.HEADS, 0.1
    g = torch.Generator().manual_seed(8)
    qkv, dout = torch.randn(B * N, 3 * h * hd, generator=g).to(cdt), torch.randn(B * N, h * hd, generator=g).to(cdt)
    seed = torch.tensor([0x5EED5EED5EED], dtype=torch.int64, device="cuda")
    assert seq_ops._global_fused(qkv, N) == (cdt == BF) and not seq_ops.plain_attention_pads(cdt, N)
    drop = (seed, p)
    a, aux = seq_ops.plain_attention_fwd(qkv.cuda(), B, N, h, drop=drop)
    dqkv = seq_ops.plain_attention_bwd(qkv.cuda(), a, dout.cuda(), aux, B, N, h, drop=drop)
    gate = 2e-2 if cdt == BF else 1e-4
    for sd_, ok in ((int(seed[0]), True), (int(seed[0]) + 1, False)):
        o_r, _, dq_r = A.attention_ref(qkv, B, N, h, hd, keep=A.keep_mask(sd_, B, h, N, p), p=p, dout=dout)
        eo = float((a.double().cpu() - o_r).abs().max() / o_r.abs().max())
        eg = float((dqkv.double().cpu() - dq_r).abs().max() / dq_r.abs().max())
        print(f"\n{cdt} mask of seed {'' if ok else '+ 1'}: out {eo:.2e} dqkv {eg:.2e} (gate {gate:.0e})")
        assert (eo < gate and eg < gate) if ok else (eo > 3 * gate and eg > 3 * gate)


def test_padded_attention_refuses_dropout():
    """float32 at 42 tokens pads the token count: attention dropout is refused there, by the module before any launch (naming
    the rate and N) and by the launch sequence itself; without that rate the block trains"""
    import htrvt_amd  # noqa: F401
    from htrvt_amd import conformer, seq_ops
    x = torch.randn(2, 42, 64, device="cuda")
    blk = conformer.ConformerBlock(64, 2, 42, ff_dropout=0.1, attn_dropout=0.1, drop_path=0.2).cuda()
    with pytest.raises(NotImplementedError, match=r"attn_dropout = 0\.1 .*N = 42 "):
        blk.train()(x)
    assert blk.last_drop_seeds is None
    qkv = torch.randn(2 * 42, 3 * 64, device="cuda")
    with pytest.raises(NotImplementedError, match="N = 42"):
        seq_ops.plain_attention_fwd(qkv, 2, 42, 2, drop=(torch.zeros(1, dtype=torch.int64, device="cuda"), 0.1))
    blk.attn.attn_drop.p = 0.0
    xr = x.clone().requires_grad_(True)
    blk.train()(xr).sum().backward()
    assert blk.last_drop_seeds.shape == (9,) and bool(torch.isfinite(xr.grad).all())
    with torch.no_grad():
        blk.eval()(x)
