"""Operands, layouts and references for the unit tests of the few-row GEMM (K2r,
rows_gemm_kernel through mq_debug_rows_gemm) and the few-row tail (ln_pool_kernel through
mq_debug_ln_pool): test_rows_gemm_cases.py on the CPU, test_gpu_rows_gemm.py on the GPU.  A
plain module.

frag16 (restated from the layout comment above frag16_image_kernel in csrc/encoder.hip): a
[R][C] matrix as 16 x 16 blocks, block (rb, cb) with cb fastest, 256 floats each; inside a
block lane l = r + 16 kq holds the float4 of row r, columns 4 kq .. 4 kq + 3, so element (r, c)
sits at float (r + 16 (c >> 2)) * 4 + (c & 3).  A V^T block (FL_OT) holds its transpose.

The four kinds are the four launches of forward_rows:
  qkv    out = LN(a) W^T + b, a = the sum of s_in planes or the embedding gather (s_in 0)
  up     out = GELU(LN(a) W^T + b), written in frag16
  oproj  out = A W^T + b + resid, A row-major with row stride lda
  down   A in frag16; plane z = A[:, Kz] W[:, Kz]^T (+ b + resid for z = 0)

Operand classes (all seeded):
  integer  (oproj, down) A, W, bias, resid integers in [-3, 3]: |sum| <= 9 * 4096 + 6 < 2^24,
           every partial sum is exact in fp32 in any order, the expected planes are exact.
  select   (qkv, up) every W row is +-e_k, k walking the 16-deep blocks of the whole depth, so
           out[r, n] = fl(+-LN(a)[r, k_n] + b[n]) bit for bit of the kernel's own ln_out.
  randn    A ~ N(0,1), W ~ 0.05 N(0,1), bias and resid ~ N(0,1).
  rows     (LN kinds) pre-LayerNorm rows of std 1 whose mean / std cycles through 0, 1, 30;
           every fifth row has one column at 50 std (BERT's outlier channel).
  gather   (qkv, s_in 0) vocab 50, type_vocab 2, ids and types out of range on both sides.
LayerNorm weights everywhere: gamma ~ 1 + 0.2 N, beta ~ 0.1 N, eps 1e-12.
"""
import functools
import math

import numpy as np

KINDS = ("qkv", "up", "oproj", "down")
LN_KINDS = ("qkv", "up")
CLASSES = ("integer", "select", "randn", "rows", "gather")
EPS = 1e-12
VOCAB, TYPE_VOCAB = 50, 2


# --------------------------------------------------------------------- frag16 ----
def frag16_offset(row, col, cols):
    """Float offset of element (row, col) of a [R][cols] matrix in its frag16 image."""
    return ((row >> 4) * (cols >> 4) + (col >> 4)) * 256 + ((row & 15) + 16 * ((col & 15) >> 2)) * 4 + (col & 3)


def _offsets(rows, cols, vt_from=None):
    """[rows][cols] float offsets; columns >= vt_from lie in transposed blocks."""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    if vt_from is not None:
        vt = c >= vt_from
        r, c = np.where(vt, (r & ~15) | (c & 15), r), np.where(vt, (c & ~15) | (r & 15), c)
    return frag16_offset(r, c, cols)


def padded_rows(M):
    return (M + 15) // 16 * 16


def encode(A):
    """The frag16 image of A [M][C] (C % 16 == 0) as a flat float32 buffer of whole 16-row
    blocks; the pad rows of the last block are NaN."""
    A = np.asarray(A, np.float32)
    M, C = A.shape
    assert C % 16 == 0
    full = np.full((padded_rows(M), C), np.nan, np.float32)
    full[:M] = A
    buf = np.empty(full.size, np.float32)
    buf[_offsets(full.shape[0], C).ravel()] = full.ravel()
    return buf


def decode(buf, M, N, vt_from=None):
    """Rows 0 .. M - 1 of the [.][N] matrix whose frag16 image is buf; the blocks at columns
    >= vt_from are stored transposed (FL_OT: vt_from = 2 N / 3)."""
    return np.asarray(buf).ravel()[_offsets(M, N, vt_from)]


# ----------------------------------------------------------------------- GELU ----
def gelu_erf_f64(x):
    """x Phi(x) = x / 2 erfc(-x / sqrt 2) in float64 (no 1 + erf cancellation below 0)."""
    import torch
    x = np.asarray(x, np.float64)
    return x * 0.5 * torch.special.erfc(torch.tensor(-x / math.sqrt(2.0))).numpy()


def gelu_tanh_f64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_f64(x, tanh):
    return gelu_tanh_f64(x) if tanh else gelu_erf_f64(x)


def gelu_f32_torch(x, tanh):
    """The plain torch-CPU float32 formula (what the oracle computes)."""
    import torch
    t = torch.tensor(np.asarray(x, np.float32))
    return torch.nn.functional.gelu(t, approximate="tanh" if tanh else "none").numpy()


_F = np.float32


def _fma(a, b, c):
    """fl32(a * b + c) of float32 arrays: the product of two float32 is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_F)


def _exp2(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(np.asarray(x, np.float64)).astype(_F)


def _rcp(x):
    with np.errstate(over="ignore", divide="ignore"):
        return (1.0 / np.asarray(x, np.float64)).astype(_F)


_ERFC_COEF = (0.17087277, -0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418,
              0.37409196, 1.00002368, -1.26551223)


def gelu_erf_f32_restated(x):
    """gelu_erf of csrc/gemm_epi.hpp step by step in float32, rcp and exp2 correctly rounded."""
    x = np.asarray(x, _F)
    z = np.abs(x) * _F(0.70710678118654752)
    t = _rcp(_fma(_F(0.5), z, _F(1.0)))
    p = np.full_like(x, _F(_ERFC_COEF[0]))
    for c in _ERFC_COEF[1:]:
        p = _fma(p, t, _F(c))
    e = t * _exp2(_fma(-z, z, p) * _F(1.4426950408889634))
    return x * np.where(x >= 0, _fma(_F(-0.5), e, _F(1.0)), _F(0.5) * e)


def gelu_tanh_f32_restated(x):
    """gelu_tanh of csrc/gemm_epi.hpp step by step in float32."""
    x = np.asarray(x, _F)
    u = _F(0.7978845608028654) * _fma(_F(0.044715) * x, x * x, x)
    with np.errstate(over="ignore"):
        return x * _rcp(_F(1.0) + _exp2(u * _F(-2.8853900817779268)))


def gelu_sweep():
    """The arguments of the GELU sweep (float32): 4096 points over [-12, 12], 1024 over
    [-1, 1], +-0, +-1e-30 and +-{13, 20, 40}."""
    extra = [0.0, -0.0, 1e-30, -1e-30, 13, -13, 20, -20, 40, -40]
    return np.concatenate([np.linspace(-12, 12, 4096), np.linspace(-1, 1, 1024), extra]).astype(_F)


GELU_REL_BOUND = 3.4e-6   # 2 x the 1.7e-6 gemm_epi.hpp documents, where |gelu| > 1e-3
GELU_REL_FLOOR = 1e-3


@functools.lru_cache(maxsize=None)
def gelu_abs_bound(tanh):
    """2 x the max |error| of the plain torch-CPU float32 formula on the sweep."""
    x = gelu_sweep()
    return 2.0 * float(np.abs(gelu_f32_torch(x, tanh).astype(np.float64) - gelu_f64(x, tanh)).max())


def gelu_errors(got, x, tanh):
    """-> (max |got - f64|, max relative error where |gelu| > 1e-3) for float32 arguments x."""
    ref = gelu_f64(x, tanh)
    err = np.abs(np.asarray(got, np.float64) - ref)
    big = np.abs(ref) > GELU_REL_FLOOR
    rel = float((err[big] / np.abs(ref[big])).max()) if big.any() else 0.0
    return float(err.max()), rel


# ------------------------------------------------------------------ operands ----
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def ln_weights(K, seed=0):
    r = _rng(11, K, seed)
    g = (1 + 0.2 * r.standard_normal(K)).astype(_F)
    b = (0.1 * r.standard_normal(K)).astype(_F)
    return g, b


def rows_class(M, K, seed=0):
    """Pre-LayerNorm rows: std 1, mean / std cycling 0, 1, 30; every fifth row one column at 50 std."""
    r = _rng(12, M, K, seed)
    x = r.standard_normal((M, K))
    x += np.array([0.0, 1.0, 30.0])[np.arange(M) % 3][:, None]
    for i in range(0, M, 5):
        x[i, r.integers(0, K)] += 50.0
    return x.astype(_F)


def split_planes(x, s_in, seed=0):
    """s_in float32 planes [s_in][M][K] whose in-order float32 sum is close to x (planes past
    the first are N(0,1); the first carries the rest)."""
    r = _rng(13, x.shape[0], x.shape[1], s_in, seed)
    planes = [r.standard_normal(x.shape).astype(_F) for _ in range(s_in - 1)]
    first = x.astype(np.float64) - sum(p.astype(np.float64) for p in planes) if planes else x
    return np.stack([np.asarray(first, _F)] + planes)


def select_columns(N, K, seed=0):
    """k_n and sign_n of the select class: column n reads depth k_n = 16 * block + offset, the
    block walking all K / 16 blocks (7 is coprime to every block count in use)."""
    r = _rng(14, N, K, seed)
    nblk = K // 16
    assert math.gcd(7, nblk) == 1
    k = ((np.arange(N) * 7 + 3) % nblk) * 16 + r.integers(0, 16, N)
    sign = r.integers(0, 2, N).astype(_F) * 2 - 1
    return k, sign


GATHER_IDS = (-5, 0, VOCAB - 1, VOCAB, VOCAB + 7)
GATHER_TYPES = (-1, 0, 1, 2)


@functools.lru_cache(maxsize=32)
def build(kind, cls, M, N, K, s_in=1, splits=1, L=0, with_types=True, seed=0):
    """-> dict of read-only operands.  LN kinds: planes [s_in][M][K] (or word / pos / typ / ids /
    types for s_in 0), g, b.  All: W [N][K], bias [N].  oproj / down: A [M][K], resid [M][N].
    select: k, sign.  Cached: callers must not write into the arrays."""
    assert kind in KINDS and cls in CLASSES
    assert (cls in ("integer",)) <= (kind in ("oproj", "down"))
    assert (cls in ("select", "rows", "gather")) <= (kind in LN_KINDS)
    r = _rng(15, KINDS.index(kind), CLASSES.index(cls), M, N, K, s_in, splits, seed)
    c = dict(kind=kind, cls=cls, M=M, N=N, K=K, s_in=s_in, splits=splits, L=L)
    if cls == "integer":
        c["A"] = r.integers(-3, 4, (M, K)).astype(_F)
        c["W"] = r.integers(-3, 4, (N, K)).astype(_F)
        c["bias"] = r.integers(-3, 4, N).astype(_F)
        c["resid"] = r.integers(-3, 4, (M, N)).astype(_F)
    else:
        if cls == "select":
            c["k"], c["sign"] = select_columns(N, K, seed)
            W = np.zeros((N, K), _F)
            W[np.arange(N), c["k"]] = c["sign"]
            c["W"] = W
        else:
            c["W"] = (0.05 * r.standard_normal((N, K))).astype(_F)
        c["bias"] = r.standard_normal(N).astype(_F)
        if kind in LN_KINDS:
            c["g"], c["b"] = ln_weights(K, seed)
            if cls == "gather":
                assert kind == "qkv" and s_in == 0 and L > 0 and M % L != 0
                c["word"] = r.standard_normal((VOCAB, K)).astype(_F)
                c["pos"] = (0.5 * r.standard_normal((L, K))).astype(_F)
                c["typ"] = (0.5 * r.standard_normal((TYPE_VOCAB, K))).astype(_F)
                ids = r.integers(0, VOCAB, M).astype(np.int32)
                at = r.permutation(M)[:len(GATHER_IDS)]
                ids[at] = GATHER_IDS[:at.size]
                c["ids"] = ids
                if with_types:
                    types = r.integers(0, TYPE_VOCAB, M).astype(np.int32)
                    at = r.permutation(M)[:len(GATHER_TYPES)]
                    types[at] = GATHER_TYPES[:at.size]
                    c["types"] = types
                else:
                    c["types"] = None
            else:
                assert s_in >= 1
                x = r.standard_normal((M, K)).astype(_F) if cls == "randn" else rows_class(M, K, seed)
                c["planes"] = split_planes(x, s_in, seed)
        else:
            c["A"] = r.standard_normal((M, K)).astype(_F)
            c["resid"] = r.standard_normal((M, N)).astype(_F)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---------------------------------------------------------------- references ----
def clamp_ids(ids, n):
    return np.clip(np.asarray(ids, np.int64), 0, n - 1)


def ln_input(c, dtype):
    """The pre-LayerNorm rows [M][K] of an LN-kind case in `dtype` (numpy): the planes summed
    in order, or the embedding sum word[id] + pos[row % L] + typ[type] with clamped ids / types."""
    if c["s_in"] == 0:
        M = c["M"]
        ids = clamp_ids(c["ids"], VOCAB)
        tt = np.zeros(M, np.int64) if c["types"] is None else clamp_ids(c["types"], TYPE_VOCAB)
        return (c["word"].astype(dtype)[ids] + c["pos"].astype(dtype)[np.arange(M) % c["L"]]) + c["typ"].astype(dtype)[tt]
    x = c["planes"][0].astype(dtype)
    for p in c["planes"][1:]:
        x = x + p.astype(dtype)
    return x


def layernorm_f64(x, g, b, eps=EPS):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def layernorm_f32_torch(x, g, b, eps=EPS):
    import torch
    t = torch.tensor(np.asarray(x, _F))
    return torch.nn.functional.layer_norm(t, (t.shape[-1],), torch.tensor(np.asarray(g)), torch.tensor(np.asarray(b)),
                                          eps).numpy()


def reference_f64(c, tanh=False):
    """-> (planes [splits][M][N] float64, ln_out [M][K] float64 or None)."""
    W = c["W"].astype(np.float64)
    if c["kind"] in LN_KINDS:
        a = layernorm_f64(ln_input(c, np.float64), c["g"], c["b"])
        y = a @ W.T + c["bias"]
        if c["kind"] == "up":
            y = gelu_f64(y, tanh)
        return y[None], a
    A, sp, Ks = c["A"].astype(np.float64), c["splits"], c["K"] // c["splits"]
    planes = [A[:, z * Ks:(z + 1) * Ks] @ W[:, z * Ks:(z + 1) * Ks].T for z in range(sp)]
    planes[0] = planes[0] + c["bias"] + c["resid"]
    return np.stack(planes), None


def reference_f32_torch(c, tanh=False):
    """The same as plain torch-CPU float32 ops: its error against reference_f64 is the d32
    the GPU tolerances are multiples of.  -> (planes float32, ln_out float32 or None)."""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, _F))
    W = t(c["W"])
    if c["kind"] in LN_KINDS:
        a = t(layernorm_f32_torch(ln_input(c, _F), c["g"], c["b"]))
        y = a @ W.T + t(c["bias"])
        if c["kind"] == "up":
            y = torch.nn.functional.gelu(y, approximate="tanh" if tanh else "none")
        return y[None].numpy(), a.numpy()
    A, sp, Ks = t(c["A"]), c["splits"], c["K"] // c["splits"]
    planes = [A[:, z * Ks:(z + 1) * Ks] @ W[:, z * Ks:(z + 1) * Ks].T for z in range(sp)]
    planes[0] = planes[0] + t(c["bias"]) + t(c["resid"])
    return torch.stack(planes).numpy(), None


def integer_expect(c):
    """The exact planes of an integer case, from int64 arithmetic -> float32 [splits][M][N]."""
    A, W = c["A"].astype(np.int64), c["W"].astype(np.int64)
    sp, Ks = c["splits"], c["K"] // c["splits"]
    planes = [A[:, z * Ks:(z + 1) * Ks] @ W[:, z * Ks:(z + 1) * Ks].T for z in range(sp)]
    planes[0] = planes[0] + c["bias"].astype(np.int64) + c["resid"].astype(np.int64)
    out = np.stack(planes)
    assert np.abs(out).max() < 2 ** 24
    return out.astype(_F)


def integer_bound(K):
    """Largest |partial sum| an integer case can reach at depth K: 9 K + bias + resid."""
    return 9 * K + 6


def select_argument(c, ln_out):
    """fl(+-ln_out[r, k_n] + bias[n]) in float32 [M][N]: a select case's exact GEMM output."""
    return np.asarray(ln_out, _F)[:, c["k"]] * c["sign"] + c["bias"]


# ------------------------------------------------------------ hook arguments ----
ROWS_GEMM_ARGS = ("kind", "variant", "A", "lda", "a_plane", "s_in", "W", "bias", "resid", "ldr", "out", "o_plane",
                  "M", "N", "K", "splits", "ln_g", "ln_b", "eps", "ln_out", "ids", "types", "L", "vocab", "pos", "typ",
                  "type_vocab", "nt_w", "zbuf", "zn", "stream")
_ROWS_GEMM_DEFAULTS = dict(variant=0, lda=0, a_plane=0, s_in=1, resid=None, ldr=0, o_plane=0, splits=1, ln_g=None,
                           ln_b=None, eps=EPS, ln_out=None, ids=None, types=None, L=1, vocab=VOCAB, pos=None, typ=None,
                           type_vocab=TYPE_VOCAB, nt_w=0, zbuf=None, zn=0, stream=None)


def rows_gemm_args(**kw):
    """mq_debug_rows_gemm's positional arguments from keywords (pointers already converted)."""
    unknown = set(kw) - set(ROWS_GEMM_ARGS)
    assert not unknown, unknown
    a = dict(_ROWS_GEMM_DEFAULTS, **kw)
    a["kind"] = KINDS.index(a["kind"]) if isinstance(a["kind"], str) else a["kind"]
    return tuple(a[n] for n in ROWS_GEMM_ARGS)


# -------------------------------------------------------------------- ln_pool ----
def pool_mask(name, B, L):
    """int32 [B][L]: ones; prefix (lengths cycling 1 .. L); holes; dead (sequence B - 1 wholly
    masked, the others as prefix)."""
    m = np.ones((B, L), np.int32)
    if name in ("prefix", "dead"):
        for b in range(B):
            m[b, 1 + (b * 5 + L // 2) % L:] = 0
    elif name == "holes":
        r = _rng(16, B, L)
        m = (r.random((B, L)) < 0.6).astype(np.int32)
        m[np.arange(B), r.integers(0, L, B)] = 1
    if name == "dead":
        m[B - 1] = 0
    return m


def ln_pool_f64(planes, mask, B, L, rows, mean, g, b, raw, eps=EPS):
    """float64 tail: LN(sum of planes) of the pooled rows, CLS row or masked mean (count
    clamped to >= 1), L2-normalised unless raw (norm clamped to >= 1e-12)."""
    x = np.asarray(planes, np.float64).sum(0).reshape(B, rows, -1)
    if mean:
        m = np.asarray(mask, np.float64).reshape(B, L, 1)
        y = (layernorm_f64(x, g, b, eps) * m).sum(1) / np.maximum(m.sum(1), 1.0)
    else:
        y = layernorm_f64(x[:, 0], g, b, eps)
    if not raw:
        y = y / np.maximum(np.sqrt((y * y).sum(-1, keepdims=True)), 1e-12)
    return y


def ln_pool_f32_torch(planes, mask, B, L, rows, mean, g, b, raw, eps=EPS):
    import torch
    p = torch.tensor(np.asarray(planes, _F))
    x = p[0]
    for z in range(1, p.shape[0]):
        x = x + p[z]
    x = x.view(B, rows, -1)
    ln = lambda v: torch.nn.functional.layer_norm(v, (v.shape[-1],), torch.tensor(np.asarray(g)),
                                                  torch.tensor(np.asarray(b)), eps)
    if mean:
        m = torch.tensor(np.asarray(mask, _F)).view(B, L, 1)
        y = (ln(x) * m).sum(1) / m.sum(1).clamp_min(1.0)
    else:
        y = ln(x[:, 0])
    if not raw:
        y = y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return y.numpy()
