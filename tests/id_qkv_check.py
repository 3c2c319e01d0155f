"""Lever 6 (zett_set_option("id_qkv")): layer 0's Q/K/V once per distinct source id.  No GPU in here.

  * pair_qkv_ref / pair_qkv_bound / pair_qkv_emulate: one launch of pair_qkv_kernel (zett_op_fwd_pair_qkv) in float64 on the SAME
    values, its per-element bound from the float64 intermediates, and the fp32 emulation.  The kernel's operations, in its order:
        a = f32(U) + C;  b = mu * cW;  d = a - b;  v = fma(r, d, bq);  out = lo(v)
    each a single IEEE operation (U |result|, U = 2^-24), the errors of a and b pass through d unchanged and through v times |r|,
    the fma is fma_bound, the store lo_bound (tests/train_ops_check.py).
  * forward_id_qkv: the oracle's forward (oracle/hypernet_ref.py) with layer 0's q / k / v computed by the identity, 16-bit
    rounding where the device rounds: the table's pre-LayerNorm sum, the folded weight, U, and q / k / v themselves.
"""
import numpy as np
import torch

from oracle import hypernet_ref as ref
from tests import train_ops_check as tc
from tests.train_ops_check import F32, F64, U, fma_bound, lo_bound

RANGE_ACTIVATION = 2
F16_MAX, F16_INF_FROM = 65504.0, 65520.0


# ---- one launch ----------------------------------------------------------------------------------------------------------
def pair_qkv_ref(u, slot, pos, stats, c_pos, c_w, b_q, dt=F64):
    """rows in the order of slot / pos / stats -> dict(a, b, d, v): the intermediates of every element in `dt`"""
    uu, cc = u.to(dt)[slot.long()], c_pos.to(dt)[pos.long()]
    mu, r = stats.to(dt)[:, :1], stats.to(dt)[:, 1:2]
    a = uu + cc
    b = mu * c_w.to(dt)
    d = a - b
    v = r * d + b_q.to(dt)
    return dict(a=a, b=b, d=d, v=v, r=r)


def pair_qkv_bound(x, lo):
    """x: pair_qkv_ref in float64 -> (fp32 bound of v, bound of the stored 16-bit value)"""
    e_d = U * (x["a"].abs() + x["b"].abs() + x["d"].abs())
    b32 = (x["r"].abs() * e_d + fma_bound(x["r"] * x["d"], x["v"] - x["r"] * x["d"])) * (1.0 + 8.0 * U)
    return b32, lo_bound(x["v"], b32, lo)


def pair_qkv_emulate(u, slot, pos, stats, c_pos, c_w, b_q, lo):
    """the same operations in fp32 (the product and the sum of the last step rounded separately: inside fma_bound)"""
    return pair_qkv_ref(u, slot, pos, stats, c_pos, c_w, b_q, dt=F32)["v"].to(lo)


def check_pair_qkv(what, got, x, lo, key=None):
    """got [n, N] of `lo` against the float64 intermediates x.  An element whose reference lies beyond the f16 range must be the
    infinity of its sign; one within half an ulp of the largest finite value may be either.  -> True when some element overflowed"""
    b32, bnd = pair_qkv_bound(x, lo)
    v = x["v"]
    if lo != torch.float16:
        tc.check(got, v, bnd, what, key=key)
        return False
    over = v.abs() - b32 >= F16_INF_FROM
    edge = (v.abs() + b32 > F16_MAX) & ~over
    g = got.to(F64)
    assert bool((g[over] == torch.sign(v[over]) * float("inf")).all()), f"{what}: a value beyond the f16 range was not stored as inf"
    keep = ~(over | edge)
    tc.check(torch.where(keep, g, v), v, bnd, what, key=key)
    return bool(over.any())


# ---- the whole forward ---------------------------------------------------------------------------------------------------
def _lo(a, kind):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if kind == "f16":
        return a.astype(np.float16).astype(np.float32)
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


def forward_id_qkv(W, cfg, ids, source_embeddings, kind="f16"):
    """hypernet_ref.forward for a configuration WITHOUT a language position, layer 0's q / k / v by the identity:
        qkv = lo( r_x ((U + C[p]) - mu_x cW) + bq ),   U = lo( r_t (lo(raw) W''^T - mu_t colsum(W'')) + (beta_t gamma) W^T ),
        W'' = lo(gamma_t gamma W),  C[p] = (type0 + pos[p]) (gamma W)^T,  cW = colsum(gamma W),  bq = beta W^T + b.
    Everything else is the oracle's own arithmetic (fp32)."""
    assert not cfg.get("hn_embed_lang_id", False)
    f32 = np.float32
    ids = np.asarray(ids).astype(np.int64)
    n, seq = ids.shape
    x = ref.embed_inputs(W, cfg, ids, source_embeddings)
    x = ref.linear(x, W["input_projection.0.weight"], W["input_projection.0.bias"])
    pfx = "input_projection.1."
    hdn = ref.gelu_tanh(ref.linear(x, W[pfx + "dense1.weight"], W[pfx + "dense1.bias"]))
    raw = ref.gelu_tanh(ref.linear(hdn, W[pfx + "dense2.weight"], W[pfx + "dense2.bias"])) + x          # the table's pre-LayerNorm sum
    g_t, b_t = W[pfx + "ln.weight"], W[pfx + "ln.bias"]
    mu_t = raw.mean(-1, keepdims=True, dtype=f32)
    r_t = 1.0 / np.sqrt(((raw - mu_t) ** 2).mean(-1, keepdims=True, dtype=f32) + f32(ref.PROJECTOR_LN_EPS))
    raw16 = _lo(raw, kind)
    t = (raw16 - mu_t) * r_t * g_t + b_t
    e = "model.embeddings."
    tt, pos_emb = W[e + "token_type_embeddings.weight"][0], W[e + "position_embeddings.weight"]
    g, b = W[e + "LayerNorm.weight"], W[e + "LayerNorm.bias"]
    c_p = tt + pos_emb[np.arange(seq)]
    emb = t + c_p
    mu_x = emb.mean(-1, keepdims=True, dtype=f32)
    r_x = 1.0 / np.sqrt(((emb - mu_x) ** 2).mean(-1, keepdims=True, dtype=f32) + f32(ref.ROBERTA_LN_EPS))
    z = ((emb - mu_x) * r_x * g + b).astype(f32)
    a0 = "model.encoder.layer.0.attention.self."
    Wq = np.concatenate([W[a0 + nm + ".weight"] for nm in ("query", "key", "value")], 0)
    bq0 = np.concatenate([W[a0 + nm + ".bias"] for nm in ("query", "key", "value")], 0)
    W2 = _lo(Wq * (g_t * g), kind)
    u = _lo(r_t * (raw16 @ W2.T - mu_t * W2.sum(1)) + (b_t * g) @ Wq.T, kind)
    W1 = (Wq * g).astype(f32)
    qkv = _lo(r_x * ((u + c_p @ W1.T) - mu_x * W1.sum(1)) + (b @ Wq.T + bq0), kind)
    hidden = _encoder(W, cfg, z, ids != int(cfg["pad_token_id"]), qkv)
    return ref._heads(W, cfg, hidden[:, 0])


def _encoder(W, cfg, z, key_mask, qkv0):
    """hypernet_ref.roberta_encoder behind its embeddings, layer 0's [q | k | v] given"""
    n, lp, hdim = z.shape
    heads = int(cfg.get("hn_num_attention_heads") or hdim // 64)
    d = hdim // heads
    bias = np.where(key_mask, np.float32(0.0), np.finfo(np.float32).min).astype(np.float32)[:, None, None, :]
    for layer in range(int(cfg.get("hn_n_layers", 3))):
        lpfx = f"model.encoder.layer.{layer}."
        a = lpfx + "attention.self."
        if layer == 0:
            q, k, v = (qkv0[..., i * hdim:(i + 1) * hdim] for i in range(3))
        else:
            q, k, v = (ref.linear(z, W[a + nm + ".weight"], W[a + nm + ".bias"]) for nm in ("query", "key", "value"))
        q, k, v = (t.reshape(n, lp, heads, d).transpose(0, 2, 1, 3) for t in (q, k, v))
        s = (q @ k.transpose(0, 1, 3, 2)).astype(np.float32) * np.float32(d ** -0.5) + bias
        s = s - s.max(axis=-1, keepdims=True)
        ex = np.exp(s).astype(np.float32)
        prob = ex / ex.sum(axis=-1, keepdims=True, dtype=np.float32)
        ctx = (prob @ v).astype(np.float32).transpose(0, 2, 1, 3).reshape(n, lp, hdim)
        o = lpfx + "attention.output."
        z = ref.layer_norm(ref.linear(ctx, W[o + "dense.weight"], W[o + "dense.bias"]) + z, W[o + "LayerNorm.weight"], W[o + "LayerNorm.bias"], ref.ROBERTA_LN_EPS)
        inter = ref.gelu_erf(ref.linear(z, W[lpfx + "intermediate.dense.weight"], W[lpfx + "intermediate.dense.bias"]))
        o = lpfx + "output."
        z = ref.layer_norm(ref.linear(inter, W[o + "dense.weight"], W[o + "dense.bias"]) + z, W[o + "LayerNorm.weight"], W[o + "LayerNorm.bias"], ref.ROBERTA_LN_EPS)
    return z
