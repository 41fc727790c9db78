"""The nine entry points of csrc/sgm.hip through the C ABI against tests/sgm_refs.py in float64, past one chunk of the
query backward (QB_ROWS = 256 rows), one block of the context kernel and the 8192-block cap of the grid-stride kernels.

Known-answer data wherever the operation allows it, so that the comparison is `torch.equal`:
  query backward   dq holds integers in [-4, 4] (exact in bfloat16; every sum is an integer below 2^16, exact in float32 in
                   any order): ddir_* equal the float64 sums, demb equals float32(sum) * float32(1 / S), vocabulary rows
                   that no id names are 0 although every output and the workspace start as NaN
  query forward    S in {1, 4}, values on the grid of multiples of 2^-6 in [-2, 2]: sum, * 1/S and + token are exact
  convert          float32 add, one round-to-nearest-even; a seventh of the float32 inputs lie on a bfloat16 tie
  context          integers
Elsewhere the gates follow tests/test_norm_kernels_gpu.py: per element against the float64 reference over the same inputs,
relative to the reference's largest magnitude, gate = 8 * E32 (+ 2^-8 |ref| for a bfloat16 output) with E32 =
kernel_refs.e32, the float32 evaluation error of the reference itself on these inputs.  The cases with logits spanning
more than +-60 add one derived term for __expf / __logf, which scale their argument x - lse in float32 (a relative
error of |x - lse| * 2^-23 of the exponential): the forward gates grow by max |x - lse| * 2^-23, the backward gate by
max (p |x - lse|) * 2^-23 * |w| / max |ref| (p = softmax, w = mask * g / den: what that error becomes in dlogits).
Nothing in a gate comes from the kernel under test.  Every comparison prints E32, gate and observed (`pytest -s`).

Measured on an MI355X, over all parametrised cases of an output (errors relative to max |ref|; a bfloat16 gate is
2^-8 = 3.9e-3 plus 8 * E32; where E32 is 0 the gate is 0 and the kernel's result was exact):

  output                            E32 (range)        worst observed   worst observed / gate
  query forward, S = 5    f32       6.4e-8 .. 7.7e-8   7.7e-8           0.13
  query forward, S = 5    bf16      6.4e-8 .. 7.7e-8   3.3e-3           0.85
  xent lse                          0 .. 6.1e-8        5.9e-8           0.29
  xent rowloss                      0 .. 8.6e-8        8.6e-8           0.15
  xent den                          0                  0                -
  xent loss                         0 .. 1.0e-7        5.4e-8           0.13 (never above E32: see below)
  xent dlogits, g only    f32       0 .. 5.7e-7        5.7e-7           0.21
  xent dlogits, with dl   f32       0 .. 1.6e-7        1.6e-7           0.13
  xent dlogits            bf16      0 .. 5.7e-7        3.6e-3           0.91
  +-60: lse / rowloss / loss        1.4e-8 .. 5.4e-8   5.4e-8 (rowloss) 0.01 (derived term 1.7e-5 .. 2.1e-5)
  +-60: dlogits           f32       0 .. 3.8e-6        3.8e-6           0.12 (derived term up to 4.4e-8)
  +-60: dlogits           bf16      0 .. 3.8e-6        3.4e-3           0.86

The scalar loss is reduced from float64 row losses and rounded once, so it is the float32 nearest the true value and
inside 8 * E32 whatever E32 is (E32 is the distance of some float32 from that value).  With float32 row losses it missed
the gate at V = 200, B = L = 1, mask ones: two rows whose float32-reference errors cancel (E32 7.9e-10, gate 6.4e-9, a
ninth of half an ulp) while the kernel's did not (7.5e-8, 1.3 ulp).
"""
import functools

import pytest
import torch

import sgm_refs as S
import kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
NAN = float("nan")
DTYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])

# (B, L, S, dtx, V): every row count (2, 256 = one chunk, 258 = a 2-row last chunk, 770 = four chunks whose edges fall inside
# a line and between the two directions of one sample), every S, every d_txt (72: a second column group of 8 live
# lanes), every V (254: the cap, 64 KB of LDS)
QUERY_CASES = [(1, 1, 1, 8, 5), (4, 32, 4, 64, 84), (3, 43, 5, 72, 254), (5, 77, 5, 256, 84), (5, 77, 4, 72, 5),
               (5, 77, 1, 64, 254), (3, 43, 1, 256, 5), (4, 32, 5, 8, 254), (1, 1, 4, 72, 84), (3, 43, 4, 8, 84)]
QUERY = pytest.mark.parametrize("B,L,Sw,dtx,V", QUERY_CASES)


def _lib():
    import htrvt_amd  # noqa: F401
    from htrvt_amd._lib import check, lib
    from htrvt_amd.ops import dt, ptr, stream
    return lib, check, ptr, stream, dt


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nan(shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _check(name, got, ref, err, bf16_out, extra=0.0):
    """kernel_refs.gate_check: gate 8 * E32 (+ one bfloat16 ulp); `extra`: a derived term added to the gate, relative to
    max |ref| like E32 (the factor stays 8)"""
    if extra:
        print(f"  {name}: E32 {err:.2e}; the next line's E32 carries the derived term {extra:.2e} / 8")
    ok, obs = R.gate_check(name, got.detach().cpu(), ref, err + extra / 8.0, bf16_out)
    assert ok, f"{name}: observed {obs:.3e} of max|ref| is outside 8 * E32 = {8 * err:.3e} + {extra:.3e}" + \
        (" + one bf16 ulp" if bf16_out else "")


def _query_ids(B, L, Sw, V, seed):
    """ids in [-3, V + 3): negatives and ids >= V are clamped by the kernel; for V >= 3 no id names row V // 2"""
    g = _gen(seed)
    ids = [torch.randint(-3, V + 3, (B, L, Sw), generator=g) for _ in range(2)]
    if V >= 3:
        ids = [torch.where(t == V // 2, t - 1, t) for t in ids]
    return g, ids[0], ids[1]


# ====================================================================== query backward
def _query_bwd(lib, ptr, stream, left, right, dq, B, L, Sw, V, dtx, dti):
    nws = lib.htrvt_sgm_query_bwd_workspace_floats(B, L, V, dtx)
    assert nws == -(-2 * B * L // 256) * (V + 2) * dtx
    ws = _nan((nws,)) if nws else None                # exactly the stated size: every slot that is read must be written
    demb, ddl, ddr = _nan((V, dtx)), _nan((dtx,)), _nan((dtx,))
    rc = lib.htrvt_sgm_query_bwd(ptr(left), ptr(right), ptr(dq), ptr(ws), ptr(demb), ptr(ddl), ptr(ddr), B, L, Sw, V, dtx, dti,
                                 stream())
    torch.cuda.synchronize()
    return rc, demb.cpu(), ddl.cpu(), ddr.cpu()


@DTYPES
@QUERY
def test_query_bwd_known_answer(B, L, Sw, dtx, V, dtype):
    lib, check, ptr, stream, dt = _lib()
    g, left, right = _query_ids(B, L, Sw, V, 1000 * L + 10 * Sw + V)
    dq = torch.randint(-4, 5, (B, 2, L, dtx), generator=g).to(dtype)
    sums, dl, dr = S.query_bwd_sums(left, right, dq.double(), V)
    assert float(sums.abs().max()) < 2 ** 16
    args = (left.cuda(), right.cuda(), dq.cuda(), B, L, Sw, V, dtx, dt(dtype))
    rc, demb, ddl, ddr = _query_bwd(lib, ptr, stream, *args)
    check(rc, "sgm_query_bwd")
    assert torch.equal(ddl.double(), dl) and torch.equal(ddr.double(), dr)
    inv_s = torch.tensor(1.0, dtype=F32) / torch.tensor(float(Sw), dtype=F32)
    assert torch.equal(demb, sums.float() * inv_s)
    if V >= 3:                                        # written, not added: the outputs started as NaN
        unused = V // 2
        assert not (torch.stack([left, right]).clamp(0, V - 1) == unused).any() and not sums[unused].any()
        assert torch.equal(demb[unused], torch.zeros(dtx))
    rc2, demb2, ddl2, ddr2 = _query_bwd(lib, ptr, stream, *args)
    assert rc2 == 0 and torch.equal(demb, demb2) and torch.equal(ddl, ddl2) and torch.equal(ddr, ddr2)


@DTYPES
def test_query_bwd_no_rows_writes_zeros(dtype):
    lib, check, ptr, stream, dt = _lib()
    for B, L in ((2, 0), (0, 3)):
        assert lib.htrvt_sgm_query_bwd_workspace_floats(B, L, 20, 24) == 0
        rc, demb, ddl, ddr = _query_bwd(lib, ptr, stream, None, None, None, B, L, 5, 20, 24, dt(dtype))
        check(rc, "sgm_query_bwd")
        assert torch.equal(demb, torch.zeros(20, 24)) and torch.equal(ddl, torch.zeros(24)) and torch.equal(ddr, torch.zeros(24))


@DTYPES
def test_query_bwd_refuses_vocabulary_above_cap(dtype):
    """V = 254 is 64 KB of LDS and runs (QUERY_CASES); one row more is refused before anything is launched"""
    lib, check, ptr, stream, dt = _lib()
    B, L, Sw, V, dtx = 1, 3, 2, 255, 8
    g, left, right = _query_ids(B, L, Sw, V, 5)
    dq = torch.randint(-4, 5, (B, 2, L, dtx), generator=g).to(dtype)
    rc, demb, ddl, ddr = _query_bwd(lib, ptr, stream, left.cuda(), right.cuda(), dq.cuda(), B, L, Sw, V, dtx, dt(dtype))
    assert rc != 0
    msg = lib.htrvt_last_error().decode()
    assert "htrvt_sgm_query_bwd" in msg and "255" in msg and "254" in msg, msg
    assert torch.isnan(demb).all() and torch.isnan(ddl).all() and torch.isnan(ddr).all()


# ====================================================================== query forward
@DTYPES
@QUERY
def test_query_fwd(B, L, Sw, dtx, V, dtype):
    lib, check, ptr, stream, dt = _lib()
    g, left, right = _query_ids(B, L, Sw, V, 1000 * L + 10 * Sw + V)
    exact = Sw in (1, 4)
    if exact:          # multiples of 2^-6 in [-2, 2]
        emb, dl, dr = (torch.randint(-128, 129, s, generator=g).float() / 64 for s in ((V, dtx), (dtx,), (dtx,)))
    else:
        emb, dl, dr = (torch.randn(s, generator=g) for s in ((V, dtx), (dtx,), (dtx,)))
    out = _nan((B, 2, L, dtx), dtype)
    dev = [t.cuda() for t in (left, right, emb, dl, dr)]
    check(lib.htrvt_sgm_query_fwd(*map(ptr, dev), ptr(out), B, L, Sw, V, dtx, dt(dtype), stream()), "sgm_query_fwd")
    out = out.cpu()
    if exact:
        ref = S.query_fwd(left, right, emb.double(), dl.double(), dr.double())
        assert torch.equal(ref.float().double(), ref)                     # exact in float32
        assert torch.equal(out, ref.float().to(dtype))                    # bfloat16: its one rounding
    else:
        print(f"\nquery_fwd {dtype} B={B} L={L} S={Sw} d_txt={dtx} V={V}")
        (ref,), (err,) = R.e32(S.query_fwd, (left, right, emb, dl, dr))
        _check("q", out, ref, err, dtype == BF)


# ====================================================================== cross-entropy
XENT_V = [(1, 1), (1, 8), (20, 20), (20, 24), (64, 64), (65, 65), (65, 72), (84, 84), (84, 88), (200, 200)]
XENT_BL = [(1, 1), (1, 3), (3, 23)]          # R = 2, 6, 138: the last block has two, two and two of its four rows


def _xent_inputs(V, ldv, B, L, mask_kind, seed, spread=3.0):
    g = _gen(seed)
    Rr = 2 * B * L
    logits = torch.full((Rr, ldv), NAN)
    logits[:, :V] = spread * torch.randn(Rr, V, generator=g)
    tgt = torch.randint(-2, V + 2, (B, L), generator=g)
    mask = {"ones": torch.ones(B, L), "zero": torch.zeros(B, L), "mixed": (torch.rand(B, L, generator=g) < 0.6).float()}[mask_kind]
    gout = torch.randn((), generator=g) + 2.0
    dl_l, dl_r = torch.randn(B, L, V, generator=g), torch.randn(B, L, V, generator=g)
    return logits, tgt, mask, gout, dl_l, dl_r


def _xent_fwd(lib, ptr, stream, logits, ldv, V, B, L, tgt, mask, copies=True):
    Rr = 2 * B * L
    ll, lr = (_nan((B, L, V)), _nan((B, L, V))) if copies else (None, None)
    lse, rowloss, loss, den = _nan((Rr,)), _nan((Rr,)), _nan(()), _nan((1,))
    scratch = _nan((Rr,), F64)
    rc = lib.htrvt_sgm_xent_fwd(ptr(logits), ldv, V, B, L, ptr(tgt), ptr(mask), ptr(ll), ptr(lr), ptr(lse), ptr(rowloss), ptr(scratch),
                                ptr(loss), ptr(den), stream())
    assert rc == 0, lib.htrvt_last_error().decode()
    return ll, lr, lse, rowloss, loss, den


def _xent_case(V, ldv, B, L, mask_kind, seed, spread=3.0, expf_term=False):
    lib, check, ptr, stream, dt = _lib()
    print(f"\nxent V={V} ldv={ldv} B={B} L={L} mask={mask_kind} spread={spread}")
    logits, tgt, mask, gout, dl_l, dl_r = _xent_inputs(V, ldv, B, L, mask_kind, seed, spread)
    d = {n: t.cuda() for n, t in dict(logits=logits, tgt=tgt, mask=mask, gout=gout, dl_l=dl_l, dl_r=dl_r).items()}
    ll, lr, lse, rowloss, loss, den = _xent_fwd(lib, ptr, stream, d["logits"], ldv, V, B, L, d["tgt"], d["mask"])
    # ---- forward
    x4 = logits.view(B, 2, L, ldv)[..., :V]
    assert torch.equal(ll.cpu(), x4[:, 0]) and torch.equal(lr.cpu(), x4[:, 1])
    ref, err = R.e32(S.xent_fwd, (logits, V, B, L, tgt, mask))
    extra = 0.0
    if expf_term:      # max |x - lse| * 2^-23: the float32 scaling of the intrinsics' argument
        extra = float((logits[:, :V].double() - ref[0][:, None]).abs().max()) * 2.0 ** -23
    for n, got, r, e in zip(("lse", "rowloss", "loss", "den"), (lse, rowloss, loss, den.reshape(())), ref, err):
        _check(n, got, r, e, False, 0.0 if n == "den" else extra)
    if mask_kind == "zero":
        assert float(den) == 2.0 and float(loss) == 0.0
    # NULL copies are accepted and change nothing; a second call is bitwise the first
    _, _, lse2, rowloss2, loss2, den2 = _xent_fwd(lib, ptr, stream, d["logits"], ldv, V, B, L, d["tgt"], d["mask"], copies=False)
    assert torch.equal(lse, lse2) and torch.equal(rowloss, rowloss2) and torch.equal(loss, loss2) and torch.equal(den, den2)
    # ---- backward: g given / NULL, the logits gradients given / NULL, both output dtypes
    p = torch.exp(logits[:, :V].double() - ref[0][:, None])
    for dtype in (F32, BF):
        for with_g in (True, False):
            for with_dl in (True, False):
                dlog = _nan((2 * B * L, ldv), dtype)
                gl, gr = (d["dl_l"], d["dl_r"]) if with_dl else (None, None)
                rc = lib.htrvt_sgm_xent_bwd(ptr(d["logits"]), ldv, V, B, L, ptr(d["tgt"]), ptr(d["mask"]), ptr(lse), ptr(den),
                                            ptr(d["gout"]) if with_g else None, ptr(gl), ptr(gr), ptr(dlog), dt(dtype), stream())
                assert rc == 0, lib.htrvt_last_error().decode()
                dlog = dlog.cpu()
                assert not dlog[:, V:].any() and not torch.isnan(dlog).any()          # the padding columns: exactly zero
                a = (logits, V, B, L, tgt, mask, gout if with_g else None, dl_l if with_dl else None, dl_r if with_dl else None)
                (rb,), (eb,) = R.e32(S.xent_bwd, a)
                if (mask_kind == "zero" or not with_g) and not with_dl:
                    assert not rb.any() and not dlog.any()                           # exactly zero everywhere
                    continue
                extra_b = 0.0
                if expf_term and with_g:
                    w = float(mask.max()) * abs(float(gout)) / float(ref[3])
                    extra_b = float((p * (logits[:, :V].double() - ref[0][:, None]).abs()).max()) * 2.0 ** -23 * w / float(rb.abs().max())
                _check(f"dlogits {'bf16' if dtype == BF else 'f32'} g={int(with_g)} dl={int(with_dl)}", dlog, rb, eb, dtype == BF,
                       extra_b)


@pytest.mark.parametrize("mask_kind", ["ones", "mixed", "zero"])
@pytest.mark.parametrize("B,L", XENT_BL)
@pytest.mark.parametrize("V,ldv", XENT_V)
def test_xent_against_float64(V, ldv, B, L, mask_kind):
    _xent_case(V, ldv, B, L, mask_kind, 100 * V + ldv + L)


@pytest.mark.parametrize("V,ldv", [(20, 24), (200, 200)])
def test_xent_needs_max_subtraction(V, ldv):
    """logits spanning more than +-60: exp(x) itself overflows float32 above 88 and a row's small terms vanish beside
    exp(60), so lse and the softmax are right only with the row maximum subtracted"""
    logits = _xent_inputs(V, ldv, 3, 23, "mixed", 7, spread=25.0)[0][:, :V]
    assert float(logits.max()) > 60 and float(logits.min()) < -60
    _xent_case(V, ldv, 3, 23, "mixed", 7, spread=25.0, expf_term=True)


# ====================================================================== convert
def _tie_values(n, g):
    """float32 values, every seventh exactly half way between two bfloat16 numbers"""
    x = torch.randn(n, generator=g) * 3
    bits = x.view(torch.int32)
    tie = (bits & ~0xFFFF) | 0x8000
    idx = torch.arange(n) % 7 == 0
    return torch.where(idx, tie, bits).view(F32)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("src_dtype,dst_dtype", [(F32, F32), (F32, BF), (BF, F32), (BF, BF)], ids=["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"])
def test_convert_exact(src_dtype, dst_dtype, accumulate):
    lib, check, ptr, stream, dt = _lib()
    for n in (1, 255, 8192 * 256 + 3):                # the last: beyond the 8192-block cap, the grid-stride loop
        g = _gen(n + accumulate)
        src = _tie_values(n, g).to(src_dtype).cuda()
        dst0 = (_tie_values(n + 1, g).to(dst_dtype) if accumulate else torch.full((n + 1,), NAN, dtype=dst_dtype)).cuda()
        dst = dst0.clone()
        check(lib.htrvt_sgm_convert(ptr(src), dt(src_dtype), ptr(dst), dt(dst_dtype), n, accumulate, stream()), "sgm_convert")
        want = src.float() + dst0[:n].float() if accumulate else src.float()          # float32 add, one rounding
        assert torch.equal(dst[:n], want.to(dst_dtype)), n
        tail = dst[n:].view(torch.int16 if dst_dtype == BF else torch.int32)
        assert torch.equal(tail, dst0[n:].view(tail.dtype)), n                         # nothing past n
    assert lib.htrvt_sgm_convert(None, dt(src_dtype), None, dt(dst_dtype), 0, accumulate, stream()) == 0


# ====================================================================== context
CONTEXT_LENGTHS = [60, 0, 1, 4, 5, 7, 8, 2, 33, 59, 17, 0]          # 0, 1, S-1 and S of every S below, the longest 60


@functools.lru_cache(maxsize=None)
def _context_lines():
    g = _gen(12)
    return tuple(tuple(torch.randint(0, 79, (n,), generator=g).tolist()) for n in CONTEXT_LENGTHS)


@pytest.mark.parametrize("Sw", [1, 5, 8])
def test_context_three_blocks_bitwise(Sw):
    lib, check, ptr, stream, dt = _lib()
    lines = _context_lines()
    B, Lmax = len(lines), max(CONTEXT_LENGTHS)
    assert B * Lmax == 720                             # three blocks of 256 threads
    pad, eos, bos_l, bos_r = 80, 81, 82, 83
    offs = [sum(CONTEXT_LENGTHS[:b]) for b in range(B)]
    table = torch.tensor(offs + CONTEXT_LENGTHS + [i for s in lines for i in s], dtype=torch.int32).cuda()
    left, right = (torch.full((B, Lmax, Sw), -7, dtype=torch.long, device="cuda") for _ in range(2))
    tgt, mask = torch.full((B, Lmax), -7, dtype=torch.long, device="cuda"), _nan((B, Lmax))
    check(lib.htrvt_sgm_context(ptr(table), B, Lmax, Sw, pad, bos_l, bos_r, eos, ptr(left), ptr(right), ptr(tgt), ptr(mask),
                                stream()), "sgm_context")
    want = S.context_batch(lines, Sw, pad, bos_l, eos)
    for n, got, w in zip(("left", "right", "tgt", "mask"), (left, right, tgt, mask), want):
        assert got.dtype == w.dtype and torch.equal(got.cpu(), w), n
