"""Operands, masks and the float64 reference for the attention kernel unit tests
(test_attention_cases.py on the CPU, test_gpu_attention.py on the GPU).  A plain module.

Layout as the kernels read it: qkv is [B*L][3H] float32, Q | K | V columns, head h at column
h * 64 of each third; mask is [B*L] int32.  The reference is softmax over the unmasked keys
in float64; a query row whose keys are all masked gives 0 (the kernels' documented
behaviour; torch gives NaN there).

Logit classes (all seeded):
  onehot  U in {-1,+1}^(L x 64), K = 8 U, Q = 8 U[target], scale = 1/8: every product and sum
          is an exact small integer, the logit is 512 at the target and 16 x (Hamming
          distance) lower elsewhere.  expf(-104) is already 0 in fp32 and the gap is >= 112
          (min_gap checks it), so p is exactly one-hot, l = 1, every rescale / merge factor
          is exactly 0 or 1 and ctx[i] == V[target(i)] bit for bit.
  tie     as onehot, the unmasked keys paired from the two ends (first with last, ...) to
          share a K row, so a pair sits in different 32-key tiles wherever two exist:
          ctx[i] == fl(V[a] + V[b]) * 0.5 bit for bit (l = 2 summed across tiles / waves).
  flat    Q, K, V ~ N(0,1): logits of std 1.
  sharp   Q ~ 12 N(0,1): logits of std 12.
  offset  sharp with 28 e_5 added to every Q and K row: logits in the hundreds, an
          unshifted exp overflows.
In onehot / tie every MASKED key copies the sign vector of an unmasked key, so a kernel
that lets a masked key in sees it tie with a winner and the row changes.
"""
import functools

import numpy as np

DH = 64
CLASSES = ("onehot", "tie", "flat", "sharp", "offset")
EXACT = ("onehot", "tie")
MASKS = ("ones", "prefix1", "prefix_lm1", "prefix_mid", "holes", "lead32", "dead_seq")
MIN_GAP = 112.0  # expf(x) == 0 in fp32 for x <= -104


# mq_debug_attention variant -> the L that reach its code paths (B = 2, heads = 2 unless the
# variant needs more): the shapes of the GPU tests, whose operands the CPU tests check
VARIANT_L = {
    1: (1, 31, 32, 33, 65),           # one, two and three key tiles; a ragged last query tile
    2: (20, 33, 64, 97),              # wave 1 with no tile at all; one tile each; two each
    4: (40, 128, 130),                # fewer tiles than waves; one each; wave 0 taking two
    8: (100, 256, 290),               # the same for 8 waves
    12: (7, 32),                      # one wave per head (heads 12, B 3)
    16: (1, 15, 16, 17, 33, 48, 64),  # 16-key quarters empty, partly filled and full
    -1: (33, 130, 290),               # the dispatcher's own picks (B 1, heads 12)
}


def variant_shape(variant, L):
    return (3, L, 12) if variant == 12 else (1, L, 12) if variant == -1 else (2, L, 2)


def mask_fits(name, B, L):
    return {"ones": True, "prefix1": L >= 2, "prefix_lm1": L >= 3, "prefix_mid": prefix_mid_len(L) is not None,
            "holes": L >= 5, "lead32": L > 32, "dead_seq": B >= 2}[name]


def prefix_mid_len(L):
    """A prefix length strictly inside (1, L - 1) that ends inside a 16- and a 32-key tile."""
    n = L // 2 + 1
    if n % 16 == 0:
        n += 1
    return n if 1 < n < L - 1 else None


def mask_names(B, L):
    return [m for m in MASKS if mask_fits(m, B, L)]


def make_mask(name, B, L):
    """-> int32 [B, L]."""
    assert mask_fits(name, B, L), (name, B, L)
    m = np.ones((B, L), np.int32)
    if name == "prefix1":
        m[:, 1:] = 0
    elif name == "prefix_lm1":
        m[:, L - 1:] = 0
    elif name == "prefix_mid":
        m[:, prefix_mid_len(L):] = 0
    elif name == "holes":
        r = np.random.default_rng([77, L])
        for b in range(B):
            drop = r.permutation(np.arange(1, L))[:max(1, L // 5)]
            m[b, drop] = 0
    elif name == "lead32":
        m[:, :32] = 0
    elif name == "dead_seq":
        m[0, :] = 0
    return m


def _signs(r, L, mask_row, tie):
    """Sign vectors U [L][64], per-query target key [L], and for each query the list of
    unmasked keys that share the target's K row (the exact winners)."""
    U = r.integers(0, 2, (L, DH)).astype(np.float32) * 2 - 1
    live = np.flatnonzero(mask_row)
    if live.size == 0:  # dead sequence: nothing to aim at
        return U, np.zeros(L, np.int64), [[] for _ in range(L)]
    group = {int(a): [int(a)] for a in live}
    if tie:
        n = live.size
        for k in range(n // 2):
            a, b = int(live[k]), int(live[n - 1 - k])
            U[b] = U[a]
            group[a] = group[b] = [a, b]
    dead = np.flatnonzero(mask_row == 0)
    for j, d in enumerate(dead):  # a masked key that gets in ties with a winner
        U[d] = U[live[j % live.size]]
    target = np.empty(L, np.int64)
    target[live] = r.permutation(live)
    if dead.size:
        target[dead] = r.choice(live, dead.size)
    return U, target, [group[int(t)] for t in target]


@functools.lru_cache(maxsize=64)
def build(cls, B, L, heads, mask_name):
    """-> dict(qkv [B*L, 3H] f32, mask [B*L] i32, scale, H, expect (EXACT classes: the exact
    ctx [B*L, H] f32, else None), winners (EXACT: per (b, h) the per-query winner lists)).
    Cached: callers must not write into the arrays."""
    assert cls in CLASSES
    H = heads * DH
    mask = make_mask(mask_name, B, L)
    r = np.random.default_rng([CLASSES.index(cls), B, L, heads, MASKS.index(mask_name)])
    qkv = np.empty((B, L, 3, heads, DH), np.float32)
    expect = np.zeros((B, L, heads, DH), np.float32) if cls in EXACT else None
    winners = {}
    for b in range(B):
        for h in range(heads):
            V = r.standard_normal((L, DH)).astype(np.float32)
            if cls in EXACT:
                U, target, win = _signs(r, L, mask[b], cls == "tie")
                Q, K = 8 * U[target], 8 * U
                winners[b, h] = win
                for i, w in enumerate(win):
                    if len(w) == 1:
                        expect[b, i, h] = V[w[0]]
                    elif len(w) == 2:
                        expect[b, i, h] = (V[w[0]] + V[w[1]]) * np.float32(0.5)
            else:
                Q = r.standard_normal((L, DH)).astype(np.float32)
                K = r.standard_normal((L, DH)).astype(np.float32)
                if cls in ("sharp", "offset"):
                    Q = Q * np.float32(12)
                if cls == "offset":
                    Q[:, 5] += np.float32(28)
                    K[:, 5] += np.float32(28)
            qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = Q, K, V
    out = dict(qkv=qkv.reshape(B * L, 3 * H), mask=mask.reshape(B * L), scale=0.125, H=H,
               expect=None if expect is None else expect.reshape(B * L, H), winners=winners)
    for a in (out["qkv"], out["mask"], out["expect"]):
        if a is not None:
            a.setflags(write=False)
    return out


def min_gap(case, B, L, heads):
    """Smallest (winning logit - best other unmasked logit) over every query of an EXACT
    case, in float64 (the logits are exact integers); inf where no other key is live."""
    H = heads * DH
    qkv = case["qkv"].astype(np.float64).reshape(B, L, 3, heads, DH)
    mask = case["mask"].reshape(B, L)
    gap = np.inf
    for (b, h), win in case["winners"].items():
        s = case["scale"] * qkv[b, :, 0, h] @ qkv[b, :, 1, h].T
        for i, w in enumerate(win):
            if not w:
                continue
            assert all(s[i, j] == 512 for j in w)
            others = [j for j in np.flatnonzero(mask[b]) if j not in w]
            if others:
                gap = min(gap, 512 - s[i, others].max())
    assert H == case["H"]
    return gap


def attention_f64(qkv, mask, B, L, heads, scale):
    """float64 softmax(scale Q K^T over unmasked keys) V -> [B*L, H]; all keys masked -> 0."""
    x = np.asarray(qkv, np.float64).reshape(B, L, 3, heads, DH)
    keep = np.asarray(mask).reshape(B, L) != 0
    out = np.zeros((B, L, heads, DH), np.float64)
    for b in range(B):
        if not keep[b].any():
            continue
        for h in range(heads):
            s = scale * (x[b, :, 0, h] @ x[b, :, 1, h].T)
            s[:, ~keep[b]] = -np.inf
            p = np.exp(s - s.max(1, keepdims=True))
            out[b, :, h] = (p / p.sum(1, keepdims=True)) @ x[b, :, 2, h]
    return out.reshape(B * L, heads * DH)


def attention_f32_numpy(qkv, mask, B, L, heads, scale):
    """The same in plain numpy float32 (scale folded into Q first, as the kernels do) - the
    CPU check that the EXACT classes give their expected rows bit for bit."""
    x = np.asarray(qkv, np.float32).reshape(B, L, 3, heads, DH)
    keep = np.asarray(mask).reshape(B, L) != 0
    out = np.zeros((B, L, heads, DH), np.float32)
    for b in range(B):
        if not keep[b].any():
            continue
        for h in range(heads):
            s = (x[b, :, 0, h] * np.float32(scale)) @ x[b, :, 1, h].T
            s[:, ~keep[b]] = -np.inf
            p = np.exp(s - s.max(1, keepdims=True), dtype=np.float32)
            l = p.sum(1, keepdims=True, dtype=np.float32)
            out[b, :, h] = (p @ x[b, :, 2, h]) * (np.float32(1) / l)
    return out.reshape(B * L, heads * DH)


def attention_f32_torch(qkv, mask, B, L, heads, scale):
    """The same operation as plain torch-CPU float32 ops (the oracle's statement of it): its
    error against attention_f64 is the d32 the GPU tolerances are multiples of."""
    import torch
    x = torch.tensor(np.array(qkv, np.float32)).view(B, L, 3, heads, DH)
    keep = torch.as_tensor(np.asarray(mask).reshape(B, L) != 0)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))  # [B, heads, L, DH]
    bias = torch.zeros(B, 1, 1, L)
    bias.masked_fill_(~keep[:, None, None, :], float("-inf"))
    s = (q @ k.transpose(-1, -2)) * scale + bias
    p = torch.softmax(s, dim=-1)
    ctx = (p @ v).transpose(1, 2).reshape(B, L, heads * DH)
    ctx[~keep.any(1)] = 0  # a sequence with no key at all
    return ctx.reshape(B * L, heads * DH).numpy()


def sharp_state_dict(cfg, seed=0):
    """synthetic_state_dict with every query and key projection weight x 4: attention logits
    of std ~5 (range ~30, mean top probability ~0.6) where the plain draw gives std 0.3."""
    from mediquery_hip.weights import synthetic_state_dict
    sd = dict(synthetic_state_dict(cfg, seed))
    for name in sd:
        if name.endswith("attention.self.query.weight") or name.endswith("attention.self.key.weight"):
            sd[name] = sd[name] * np.float32(4)
    return sd
