"""MI355X-native semantic-guidance (SGM) head behind the SGM forks' Python API.

Drop-in for model/sgm_head.py of the eleven model_sgm_* forks (byte-identical in all of them):
    build_sgm_vocab(converter, add_tokens=...) -> (stoi, itos, pad_id, eos_id, bos_l_id, bos_r_id)     host code
    texts_to_ids(texts, stoi) -> list of int64 tensors                                                   host code
    make_context_batch(texts, stoi, sub_str_len=5, device='cuda') -> left, right [B, Lmax, S] int64, tgt [B, Lmax] int64,
        mask [B, Lmax] float32: one host pass over the characters, one pinned upload, one kernel (htrvt_sgm_context)
    SGMHead(d_vis, vocab_size_sgm, d_txt=256, sub_str_len=5, num_heads=8, p_drop=0.1, compute_dtype=torch.float32)
        (vis_tokens [B, N, D], left, right, tgt, mask) -> {'loss_sgm', 'logits_l', 'logits_r'}
Same module tree, names and construction order as the fork's head, so `torch.manual_seed(s); SGMHead(...)` gives its
initial state_dict.  The forward is ONE autograd node over HIP kernels (csrc/sgm.hip plus the GEMM / LayerNorm / row-softmax
kernels of the hot path): both directions run as one [B, 2L] query batch against one kv_norm(F) (the fork normalises F
twice, with the same result); the gradients are bitwise reproducible (no float atomics).  Dropout on the attention output
is active in train mode with p_drop > 0: its mask comes from a counter-based generator seeded by an int64 drawn on the
device from the CUDA default generator (the CPU generator, which draws the encoder's span mask, is not touched).
compute_dtype: torch.float32 (parity) or torch.bfloat16 (throughput: the GEMM operands and activations; LayerNorm
statistics, logits and the cross-entropy stay float32).  num_heads is accepted and unused, as in the fork.
"""
import numpy as np
import torch
import torch.nn as nn

import htrvt_amd                        # noqa: F401  (loads libhtrvt_hip.so or raises)
from htrvt_amd import seq_ops
from htrvt_amd._lib import check, lib
from htrvt_amd.ops import MNMAJOR, dt, gemm, ptr, stream
from htrvt_amd.seq_ops import convert as _convert, linear_wgrad as _wgrad

SPECIAL_TOKENS = ("<pad>", "<eos>", "<bos_left>", "<bos_right>")


def build_sgm_vocab(converter, add_tokens=SPECIAL_TOKENS):
    """the converter's symbols (no CTC blank) in order, then the special tokens that are not among them"""
    stoi = {}
    for i, ch in enumerate(converter.character):     # a repeated symbol keeps the index of its last position
        stoi[ch] = i
    for tok in add_tokens:
        if tok not in stoi:
            stoi[tok] = len(stoi)
    itos = [''] * len(stoi)
    for ch, i in stoi.items():
        itos[i] = ch
    return stoi, itos, stoi["<pad>"], stoi["<eos>"], stoi["<bos_left>"], stoi["<bos_right>"]


def texts_to_ids(texts, stoi):
    return [torch.tensor([stoi[ch] for ch in t], dtype=torch.long) for t in texts]


def make_context_batch(texts, stoi, sub_str_len=5, device='cuda'):
    """left / right context windows [B, Lmax, S] int64 (<bos_left> / <eos> where a window leaves the line), targets
    [B, Lmax] int64 and mask [B, Lmax] float32; positions past a line's end hold <pad> / 0"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("make_context_batch builds the context batch on an MI355X only (no CPU / eager fallback exists)")
    B, S = len(texts), int(sub_str_len)
    if B == 0:
        raise ValueError("make_context_batch: empty text list")
    lens = [len(t) for t in texts]
    Lmax = max(lens)
    table = np.empty(2 * B + sum(lens), dtype=np.int32)
    table[B:2 * B] = lens
    table[:B] = np.cumsum([0] + lens[:-1])
    table[2 * B:] = [stoi[ch] for t in texts for ch in t]
    dev_table = torch.from_numpy(table).pin_memory().to(device, non_blocking=True)
    left = torch.empty(B, Lmax, S, dtype=torch.long, device=device)
    right = torch.empty(B, Lmax, S, dtype=torch.long, device=device)
    tgt = torch.empty(B, Lmax, dtype=torch.long, device=device)
    mask = torch.empty(B, Lmax, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        check(lib.htrvt_sgm_context(ptr(dev_table), B, Lmax, S, stoi["<pad>"], stoi["<bos_left>"], stoi["<bos_right>"],
                                    stoi["<eos>"], ptr(left), ptr(right), ptr(tgt), ptr(mask), stream()), "sgm_context")
    return left, right, tgt, mask


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


PARAMS = ("emb.weight", "dir_left", "dir_right", "txt_proj.weight", "txt_proj.bias", "q_norm.weight", "q_norm.bias",
          "kv_norm.weight", "kv_norm.bias", "classifier.weight", "classifier.bias")


class _SGMFunction(torch.autograd.Function):
    """(vis, left, right, tgt, mask, parameters) -> (loss, logits_l, logits_r); every step a HIP kernel"""

    @staticmethod
    def forward(ctx, head, vis, left, right, tgt, mask, p_drop, need, *params):
        ctx.set_materialize_grads(False)
        P = dict(zip(PARAMS, params))
        cdt = head.compute_dtype
        dti = dt(cdt)
        dev = vis.device
        B, N, D = vis.shape
        L, S = left.shape[1], left.shape[2]
        V, dtx = P["emb.weight"].shape
        Vp = (V + 7) // 8 * 8            # classifier rows padded: 16-byte rows of the d logits GEMM operand
        R = 2 * B * L                   # query rows (b, dir, l)
        f32 = torch.float32
        left, right, tgt = left.contiguous(), right.contiguous(), tgt.contiguous()
        mask = mask.contiguous().float()
        logits_l, logits_r = _empty((B, L, V), f32, dev), _empty((B, L, V), f32, dev)
        loss, den = _empty((), f32, dev), _empty(1, f32, dev)
        lse, rowloss = _empty(max(R, 1), f32, dev), _empty(max(R, 1), f32, dev)
        rowloss64 = _empty(max(R, 1), torch.float64, dev)      # scratch: the scalar loss is reduced in float64
        st = stream()
        if R == 0:           # no character in the batch: loss 0, zero gradients
            check(lib.htrvt_sgm_xent_fwd(None, Vp, V, B, L, None, None, None, None, None, None, None, ptr(loss), ptr(den), st),
                  "sgm_xent_fwd")
            ctx.empty = True
            ctx.shapes = [t.shape for t in params] + [vis.shape]
            if not need:
                ctx.mark_non_differentiable(loss, logits_l, logits_r)
            return loss, logits_l, logits_r
        ctx.empty = False
        # weights in the compute dtype (classifier rows zero-padded to Vp); float32 uses the parameters in place
        wt = P["txt_proj.weight"].contiguous()
        if cdt != f32:
            wt = _convert(wt, _empty(wt.shape, cdt, dev))
        wc = torch.zeros(Vp, D, dtype=cdt, device=dev)
        _convert(P["classifier.weight"].contiguous(), wc[:V])
        bc = torch.zeros(Vp, dtype=f32, device=dev)
        _convert(P["classifier.bias"].contiguous(), bc[:V])
        visc = vis.contiguous().float() if cdt == f32 else _convert(vis.contiguous().float(), _empty(vis.shape, cdt, dev))

        A = _empty((R, dtx), cdt, dev)
        check(lib.htrvt_sgm_query_fwd(ptr(left), ptr(right), ptr(P["emb.weight"].contiguous()), ptr(P["dir_left"].contiguous()),
                                      ptr(P["dir_right"].contiguous()), ptr(A), B, L, S, V, dtx, dti, st), "sgm_query_fwd")
        Qp = _empty((R, D), cdt, dev)
        gemm(A, wt, Qp, dtype=cdt, M=R, N=D, K=dtx, lda=dtx, ldb=dtx, ldc=D, bias=P["txt_proj.bias"].contiguous())
        Q, qm, qr = seq_ops.layernorm_fwd(Qp, P["q_norm.weight"].contiguous(), P["q_norm.bias"].contiguous(), head.q_norm.eps)
        K, km, kr = seq_ops.layernorm_fwd(visc.view(B * N, D), P["kv_norm.weight"].contiguous(),
                                          P["kv_norm.bias"].contiguous(), head.kv_norm.eps)
        # cross-attention of both directions as one [B, 2L] query batch: softmax(Q K^T / sqrt(D)) K, K = V = kv_norm(F)
        O, Pm = seq_ops.cross_attention_fwd(Q.view(B, 2 * L, D), K.view(B, N, D))
        O = O.view(R, D)
        seed = None
        if p_drop > 0:
            seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev)     # CUDA default generator, no sync
            Od = torch.empty_like(O)
            check(lib.htrvt_sgm_dropout(ptr(O), ptr(Od), R * D, ptr(seed), float(p_drop), dti, st), "sgm_dropout")
        else:
            Od = O
        logits = _empty((R, Vp), f32, dev)
        gemm(Od, wc, logits, dtype=cdt, M=R, N=Vp, K=D, lda=D, ldb=D, ldc=Vp, bias=bc, c_f32=True)
        check(lib.htrvt_sgm_xent_fwd(ptr(logits), Vp, V, B, L, ptr(tgt), ptr(mask), ptr(logits_l), ptr(logits_r), ptr(lse),
                                     ptr(rowloss), ptr(rowloss64), ptr(loss), ptr(den), st), "sgm_xent_fwd")
        if need:
            ctx.save_for_backward(left, right, tgt, mask, A, Qp, qm, qr, Q, visc, km, kr, K, Pm, Od, logits, lse, den, wt, wc,
                                  seed, P["q_norm.weight"], P["kv_norm.weight"])
            ctx.dims = (B, N, D, L, S, V, Vp, dtx, float(p_drop), cdt)
        else:
            ctx.mark_non_differentiable(loss, logits_l, logits_r)
        return loss, logits_l, logits_r

    @staticmethod
    def backward(ctx, gloss, glog_l, glog_r):
        if ctx.empty:
            shapes = ctx.shapes
            dev = gloss.device if gloss is not None else (glog_l if glog_l is not None else glog_r).device
            zeros = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]
            return (None, zeros[-1], None, None, None, None, None, None) + tuple(zeros[:-1])
        (left, right, tgt, mask, A, Qp, qm, qr, Q, visc, km, kr, K, Pm, Od, logits, lse, den, wt, wc, seed, qg,
         kg) = ctx.saved_tensors
        B, N, D, L, S, V, Vp, dtx, p_drop, cdt = ctx.dims
        dti, dev, f32, st = dt(cdt), A.device, torch.float32, stream()
        R = 2 * B * L
        gl = None if glog_l is None else glog_l.contiguous().float()
        gr = None if glog_r is None else glog_r.contiguous().float()
        g = None if gloss is None else gloss.contiguous().float()
        dlog = _empty((R, Vp), cdt, dev)
        check(lib.htrvt_sgm_xent_bwd(ptr(logits), Vp, V, B, L, ptr(tgt), ptr(mask), ptr(lse), ptr(den), ptr(g), ptr(gl),
                                     ptr(gr), ptr(dlog), dti, st), "sgm_xent_bwd")
        dwc, dbc = _wgrad(dlog, Od, R)
        dOd = _empty((R, D), cdt, dev)
        gemm(dlog, wc, dOd, dtype=cdt, M=R, N=D, K=Vp, lda=Vp, ldb=D, ldc=D, b_layout=MNMAJOR)
        if p_drop > 0:        # the same mask, regenerated from the seed
            dO = torch.empty_like(dOd)
            check(lib.htrvt_sgm_dropout(ptr(dOd), ptr(dO), R * D, ptr(seed), p_drop, dti, st), "sgm_dropout")
        else:
            dO = dOd
        dQ, dK = seq_ops.cross_attention_bwd(Q.view(B, 2 * L, D), K.view(B, N, D), Pm, dO.view(B, 2 * L, D))
        dkn = torch.zeros(2 * D, dtype=f32, device=dev)      # (d weight | d bias) adjacent: one column-sum launch
        dvisc = seq_ops.layernorm_bwd(dK, visc.view(B * N, D), km, kr, kg, dkn[:D], dkn[D:])
        dvis = dvisc.view(B, N, D) if cdt == f32 else _convert(dvisc, _empty((B, N, D), f32, dev))
        dqn = torch.zeros(2 * D, dtype=f32, device=dev)
        dQp = seq_ops.layernorm_bwd(dQ, Qp, qm, qr, qg, dqn[:D], dqn[D:])
        dwt, dbt = _wgrad(dQp, A, R)
        dA = _empty((R, dtx), cdt, dev)
        gemm(dQp, wt, dA, dtype=cdt, M=R, N=dtx, K=D, lda=D, ldb=dtx, ldc=dtx, b_layout=MNMAJOR)
        demb = _empty((V, dtx), f32, dev)
        ddl, ddr = _empty((1, 1, dtx), f32, dev), _empty((1, 1, dtx), f32, dev)
        ws = _empty(max(lib.htrvt_sgm_query_bwd_workspace_floats(B, L, V, dtx), 1), f32, dev)
        check(lib.htrvt_sgm_query_bwd(ptr(left), ptr(right), ptr(dA), ptr(ws), ptr(demb), ptr(ddl), ptr(ddr), B, L, S, V, dtx,
                                      dti, st), "sgm_query_bwd")
        grads = (demb, ddl, ddr, dwt, dbt, dqn[:D], dqn[D:], dkn[:D], dkn[D:], dwc[:V], dbc[:V])
        return (None, dvis, None, None, None, None, None, None) + grads


class SGMHead(nn.Module):
    """Training-only semantic guidance head: predicts every character of a line from its left and its right context window,
    attending over the encoder's final-norm features; masked two-direction cross-entropy."""

    def __init__(self, d_vis, vocab_size_sgm, d_txt=256, sub_str_len=5, num_heads=8, p_drop=0.1,
                 compute_dtype=torch.float32):
        super().__init__()
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"SGMHead: compute_dtype torch.float32 or torch.bfloat16, got {compute_dtype}")
        self.vocab_size = vocab_size_sgm
        self.sub_str_len = sub_str_len
        self.emb = nn.Embedding(vocab_size_sgm, d_txt)
        self.dir_left = nn.Parameter(torch.randn(1, 1, d_txt))
        self.dir_right = nn.Parameter(torch.randn(1, 1, d_txt))
        self.txt_proj = nn.Linear(d_txt, d_vis)
        self.q_norm = nn.LayerNorm(d_vis)
        self.kv_norm = nn.LayerNorm(d_vis)
        self.dropout = nn.Dropout(p_drop)
        self.classifier = nn.Linear(d_vis, vocab_size_sgm)
        self.compute_dtype = compute_dtype

    def forward(self, vis_tokens, left_ctx_ids, right_ctx_ids, tgt_ids, tgt_mask):
        """vis_tokens [B, N, D]; left / right context ids [B, L, S]; tgt_ids [B, L]; tgt_mask [B, L] (1 real, 0 padding).
        Returns {'loss_sgm': scalar, 'logits_l': [B, L, V], 'logits_r': [B, L, V]} (float32)."""
        params = [self.get_parameter(n) for n in PARAMS]
        ins = (vis_tokens, left_ctx_ids, right_ctx_ids, tgt_ids, tgt_mask)
        if not all(t.is_cuda for t in ins + tuple(params)):
            raise RuntimeError("SGMHead runs on an MI355X only: move the head and its inputs to cuda "
                               "(no CPU / eager fallback exists)")
        B, N, D = vis_tokens.shape
        if left_ctx_ids.shape != right_ctx_ids.shape or left_ctx_ids.shape[:2] != tgt_ids.shape or \
                tgt_ids.shape != tgt_mask.shape or left_ctx_ids.shape[0] != B:
            raise ValueError("SGMHead: context ids [B, L, S] (both), tgt_ids / tgt_mask [B, L] expected")
        if left_ctx_ids.dtype != torch.long or tgt_ids.dtype != torch.long:
            raise TypeError("SGMHead: context and target ids are int64")
        p_drop = float(self.dropout.p) if self.training else 0.0
        need = torch.is_grad_enabled() and (vis_tokens.requires_grad or any(p.requires_grad for p in params))
        with torch.cuda.device(vis_tokens.device):
            loss, logits_l, logits_r = _SGMFunction.apply(self, vis_tokens, left_ctx_ids, right_ctx_ids, tgt_ids, tgt_mask,
                                                          p_drop, need, *params)
        return {'loss_sgm': loss, 'logits_l': logits_l, 'logits_r': logits_r}
