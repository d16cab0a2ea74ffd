"""NumPy reference of MULTI-HEAD softmax dot-product attention over a CSR pattern (ops.spattn / ops.spattn_bwd with
``heads``; include/sgcn.h sgcn_spattn_mh_csr_f32, sgcn_spattn_mh_csr_bwd_q_f32, sgcn_spattn_mh_csr_bwd_kv_f32) -- a test-only
helper.

Definition.  heads = H >= 1, d % H == 0, dh = d / H; head h is the columns [h dh, (h + 1) dh) of Q, B, G, C, dQ, dB and the
addends.  For every head independently, over the stored pattern (unique column ids per row, values never read):
    s_ij^h     = scale * <Q_i^h, B_j^h>
    lse[i, h]  = log sum_j exp(s_ij^h)
    p_ij^h     = exp(s_ij^h - lse[i, h])
    C_i^h      = sum_j p_ij^h B_j^h                  (an empty row: +0.0 and lse = -inf in every head)
    delta[i,h] = <G_i^h, C_i^h>,   e_ij^h = p_ij^h (<G_i^h, B_j^h> - delta[i, h])
    dQ_i^h     = scale sum_j e_ij^h B_j^h (+ add)
    dB_j^h     = sum_i ( p_ij^h G_i^h + scale e_ij^h Q_i^h ) (+ add)
lse is an (M, H) table.  H = 1 is tests/spattn_ref.py exactly.

The heads do not interact, so this IS spattn_ref.forward / backward_f64 called on each head's column slices (the ``d`` of
its analysis is then dh) and concatenated: the values, lse and the derived per-element bounds.  A bound of spattn_ref holds
for a correct fp32 evaluation of a dh-wide attention, which is what every head's lanes perform; nothing is fitted here.
"""
import numpy as np

import spattn_ref as ref

U = ref.U
same_bits = ref.same_bits


def head_slices(d, heads):
    assert heads >= 1 and d % heads == 0, (d, heads)
    dh = d // heads
    return [slice(h * dh, (h + 1) * dh) for h in range(heads)]


class Forward(object):
    """C (M x d), lse (M x H), bound_C, bound_lse of the same shapes; ``per_head`` the single-head Forward objects"""


def forward(a, Q, B, scale, heads, values_only=False):
    Q, B = np.asarray(Q), np.asarray(B)
    f = Forward()
    f.per_head = [ref.forward(a, Q[:, s], B[:, s], scale, values_only) for s in head_slices(B.shape[1], heads)]
    f.C = np.concatenate([h.C for h in f.per_head], axis=1)
    f.bound_C = np.concatenate([h.bound_C for h in f.per_head], axis=1)
    f.lse = np.stack([h.lse for h in f.per_head], axis=1)
    f.bound_lse = np.stack([h.bound_lse for h in f.per_head], axis=1)
    f.deg = f.per_head[0].deg
    return f


def forward_loops(a, Q, B, scale, heads):
    """The definition entry by entry (small matrices): (C, lse), spattn_ref.forward_loops on every head's slices."""
    Q, B = np.asarray(Q), np.asarray(B)
    parts = [ref.forward_loops(a, Q[:, s], B[:, s], scale) for s in head_slices(B.shape[1], heads)]
    return np.concatenate([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1)


def loss_f64(a, Q, B, scale, G, heads):
    return float(np.sum(np.asarray(G, np.float64) * forward(a, Q, B, scale, heads).C))


def backward_f64(a, Q, B, G, scale, heads, add=None, add_rows=0, fused=False, values_only=False):
    """spattn_ref.backward_f64's dict, every array the heads' side by side; 'fwd' is this module's Forward."""
    Q, B, G = np.asarray(Q), np.asarray(B), np.asarray(G)
    M = a.shape[0]
    parts = []
    for s in head_slices(B.shape[1], heads):
        kw = dict(add=np.asarray(add)[:, s], add_rows=add_rows) if add is not None and add_rows > 0 else {}
        parts.append(ref.backward_f64(a, B[:M, s] if fused else Q[:, s], B[:, s], G[:, s], scale, fused=fused,
                                      values_only=values_only, **kw))
    out = {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0] if k != 'fwd'}
    f = Forward()
    f.per_head = [p['fwd'] for p in parts]
    f.C = np.concatenate([h.C for h in f.per_head], axis=1)
    f.bound_C = np.concatenate([h.bound_C for h in f.per_head], axis=1)
    f.lse = np.stack([h.lse for h in f.per_head], axis=1)
    f.bound_lse = np.stack([h.bound_lse for h in f.per_head], axis=1)
    f.deg = f.per_head[0].deg
    out['fwd'] = f
    return out


def forward_online_f32(a, Q, B, scale, heads, reverse=False, cut=False):
    Q, B = np.asarray(Q), np.asarray(B)
    parts = [ref.forward_online_f32(a, Q[:, s], B[:, s], scale, reverse, cut) for s in head_slices(B.shape[1], heads)]
    return np.concatenate([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1)


def backward_f32(a, Q, B, G, scale, C, lse, heads, reverse=False, cut=False):
    Q, B, G, C, lse = (np.asarray(x) for x in (Q, B, G, C, lse))
    parts = [ref.backward_f32(a, Q[:, s], B[:, s], G[:, s], scale, C[:, s], lse[:, h], reverse, cut)
             for h, s in enumerate(head_slices(B.shape[1], heads))]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
