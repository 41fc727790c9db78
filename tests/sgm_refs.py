"""Plain torch statements of the SGM head's operations (csrc/sgm.hip), in the layout the kernels use: row r of the query
batch is (b, dir, l) of [B][2][L], dir 0 = the left windows, 1 = the right windows.  Written from the header comments of
csrc/sgm.hip / include/htrvt.h and the docstring of htrvt_amd/sgm/model/sgm_head.py -- not from the kernels.

Contract of tests/kernel_refs.py: every function computes in the dtype of its floating-point inputs (float64: the yardstick;
float32: "the same operation evaluated in float32", whose distance from the yardstick scales the gates of the GPU parity
tests) and no GPU is needed to import or run it.  tests/test_sgm_refs_cpu.py anchors it to tests/golden/sgm.npz (the
reference head run in float64) and to float64 autograd.
"""
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------ context batch
def context_batch(id_lists, S, pad, bos_l, eos):
    """id_lists: B lists of character ids -> left, right [B][Lmax][S] int64, tgt [B][Lmax] int64, mask [B][Lmax] float32.
    Position i of a line sees the S characters before it (left; <bos_left> where the line has not begun) and the S after
    it (right; <eos> where it has ended); positions past a line's end hold <pad> / mask 0."""
    B, Lmax = len(id_lists), max(len(s) for s in id_lists)
    left = torch.full((B, Lmax, S), pad, dtype=torch.long)
    right = torch.full((B, Lmax, S), pad, dtype=torch.long)
    tgt = torch.full((B, Lmax), pad, dtype=torch.long)
    mask = torch.zeros(B, Lmax, dtype=torch.float32)
    for b, seq in enumerate(id_lists):
        n = len(seq)
        for i in range(n):
            tgt[b, i] = int(seq[i])
            mask[b, i] = 1.0
            for k in range(S):
                before, after = i - S + k, i + 1 + k
                left[b, i, k] = int(seq[before]) if before >= 0 else bos_l
                right[b, i, k] = int(seq[after]) if after < n else eos
    return left, right, tgt, mask


# ------------------------------------------------------------------ query: embedding gather, mean over S, + direction token
def _ids(left, right, V):
    """[B][2][L][S], clamped into [0, V)"""
    return torch.stack([left, right], dim=1).clamp(0, V - 1)


def query_fwd(left, right, emb, dir_l, dir_r):
    """left / right [B][L][S] int64, emb [V][dtx], dir_* dtx values -> [B][2][L][dtx]"""
    ids = _ids(left, right, emb.shape[0])
    tok = torch.stack([dir_l.reshape(-1), dir_r.reshape(-1)])                  # [2][dtx]
    return emb[ids].sum(3) / ids.shape[3] + tok[None, :, None, :]


def query_bwd_sums(left, right, dq, V):
    """dq [B][2][L][dtx] -> the plain sums: per vocabulary row over every (row, window slot) that holds it [V][dtx], and
    over the rows of each direction [dtx], [dtx]"""
    ids = _ids(left, right, V)
    S, dtx = ids.shape[3], dq.shape[3]
    sums = torch.zeros(V, dtx, dtype=dq.dtype)
    sums.index_add_(0, ids.reshape(-1), dq[:, :, :, None, :].expand(-1, -1, -1, S, -1).reshape(-1, dtx))
    return sums, dq[:, 0].sum((0, 1)), dq[:, 1].sum((0, 1))


def query_bwd(left, right, dq, V):
    """-> demb [V][dtx] (rows no id names are zero), ddir_l [dtx], ddir_r [dtx]"""
    sums, dl, dr = query_bwd_sums(left, right, dq, V)
    return sums / left.shape[2], dl, dr


# ------------------------------------------------------------------ masked two-direction cross-entropy
def _row_targets(V, B, L, tgt, mask):
    """per row r = (b, dir, l): the clamped target and the mask, [2 B L] each"""
    t = tgt.clamp(0, V - 1)[:, None, :].expand(B, 2, L).reshape(-1)
    return t, mask[:, None, :].expand(B, 2, L).reshape(-1)


def xent_fwd(logits, V, B, L, tgt, mask):
    """logits [2 B L][ldv] (only the first V columns are read), tgt [B][L] int64 (clamped), mask [B][L]
    -> lse [R], rowloss [R] = (lse - logit at the target) * mask, loss = sum(rowloss) / den, den = 2 max(sum(mask), 1)"""
    x = logits[:, :V]
    m = x.max(-1).values
    lse = m + torch.log(torch.exp(x - m[:, None]).sum(-1))
    t, w = _row_targets(V, B, L, tgt, mask)
    rowloss = (lse - x.gather(1, t[:, None])[:, 0]) * w
    den = 2.0 * mask.sum().clamp_min(1.0)
    return lse, rowloss, rowloss.sum() / den, den


def xent_bwd(logits, V, B, L, tgt, mask, gout=None, dl_l=None, dl_r=None):
    """-> dlogits [2 B L][ldv] = (softmax - onehot) * mask * gout / den, plus the incoming gradients dl_l / dl_r [B][L][V]
    of the returned logits copies; gout None = 0; the columns V .. ldv-1 are zero"""
    x = logits[:, :V]
    lse, _, _, den = xent_fwd(logits, V, B, L, tgt, mask)
    t, w = _row_targets(V, B, L, tgt, mask)
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    g = 0.0 if gout is None else gout.reshape(())
    d = (torch.exp(x - lse[:, None]) - onehot) * (w * g / den)[:, None]
    d = d.reshape(B, 2, L, V)
    if dl_l is not None:
        d[:, 0] = d[:, 0] + dl_l
    if dl_r is not None:
        d[:, 1] = d[:, 1] + dl_r
    out = torch.zeros_like(logits)
    out[:, :V] = d.reshape(-1, V)
    return out


# ------------------------------------------------------------------ the whole head, eval mode
def head(params, vis, left, right, tgt, mask):
    """params: the SGMHead state_dict names -> tensors of vis' dtype; vis [B][N][D] -> loss, logits_l, logits_r [B][L][V].
    query -> txt_proj -> q_norm; K = kv_norm(vis); softmax(Q K^T / sqrt(D)) K; classifier; cross-entropy."""
    B, N, D = vis.shape
    L = left.shape[1]
    V = params["emb.weight"].shape[0]
    eps = torch.nn.LayerNorm(1).eps
    q = query_fwd(left, right, params["emb.weight"], params["dir_left"], params["dir_right"])      # [B][2][L][dtx]
    q = F.linear(q, params["txt_proj.weight"], params["txt_proj.bias"]).reshape(B, 2 * L, D)
    Q = F.layer_norm(q, (D,), params["q_norm.weight"], params["q_norm.bias"], eps)
    K = F.layer_norm(vis, (D,), params["kv_norm.weight"], params["kv_norm.bias"], eps)
    P = torch.softmax(Q @ K.transpose(1, 2) / D ** 0.5, dim=-1)
    logits = F.linear(P @ K, params["classifier.weight"], params["classifier.bias"])                # [B][2L][V]
    loss = xent_fwd(logits.reshape(-1, V), V, B, L, tgt, mask.to(vis.dtype))[2]
    logits = logits.reshape(B, 2, L, V)
    return loss, logits[:, 0], logits[:, 1]
