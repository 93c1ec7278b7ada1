"""Shared helper of the cross-encoder tests (not a test module; oracle/ is frozen, so the
restatement lives here): a torch-CPU restatement of the scoring forward and the seeded pair
generator, used by tests/golden/make_cross_encoder_golden.py, the CPU tests and the GPU tests.

What it restates: transformers' BertForSequenceClassification - BertModel with token-type
ids, BertPooler (tanh(Wp h_cls + bp) on the CLS row of the last LayerNorm, not normalised) and
the classifier - pinned against transformers 5.15 by tests/golden/cross_encoder_golden.npz.
The layers are OracleEncoder's; only the embedding sum (token-type row per token) and the head
are new.
"""
import os

import numpy as np
import torch

from mediquery_hip.config import BertConfig
from mediquery_hip.weights import HEAD_NAMES, synthetic_head_state_dict, synthetic_state_dict
from oracle.encoder import OracleEncoder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLS, SEP = 101, 102
MIN_GAP = 5e-5      # smallest gap between neighbouring float64 logits of a ranking case
LOGIT_TOL = 1e-5    # |logit - float64| of every end-to-end check
# the ranking cases: (layers, B, L); the golden script finds each one's seed
RANK_CASES = [(2, 1, 8), (2, 3, 21), (2, 5, 33), (2, 9, 130), (12, 24, 64)]


class CrossOracle(OracleEncoder):
    """OracleEncoder + token types + pooler + classifier, in `dtype`."""

    def __init__(self, cfg, state_dict, head_sd, dtype=torch.float32):
        super().__init__(cfg, state_dict, dtype)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
        self.wp, self.bp, self.wc, self.bc = (t(head_sd[n]) for n in HEAD_NAMES)

    @torch.no_grad()
    def cls_states(self, ids, types, mask):
        """The CLS rows of the last LayerNorm [B, H] (OracleEncoder.hidden_states with the
        token-type row of every token instead of row 0)."""
        cfg = self.cfg
        ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
        types = torch.as_tensor(np.asarray(types), dtype=torch.long).clamp(0, cfg.type_vocab - 1)
        keep = torch.as_tensor(np.asarray(mask), dtype=torch.bool)
        B, L = ids.shape
        H, nh = cfg.hidden, cfg.heads
        dh = H // nh
        x = self._ln(self.word[ids] + self.pos[:L].unsqueeze(0) + self.typ[types], self.eln)
        bias = torch.zeros(B, 1, 1, L, dtype=self.dtype)
        bias.masked_fill_(~keep[:, None, None, :], float("-inf"))
        for w in self.layers:
            heads = lambda y: y.view(B, L, nh, dh).transpose(1, 2)
            q = heads(x @ w["wq"].T + w["bq"])
            k = heads(x @ w["wk"].T + w["bk"])
            v = heads(x @ w["wv"].T + w["bv"])
            ctx = self.attention(q, k, v, bias, dh).transpose(1, 2).reshape(B, L, H)
            x = self._ln(x + ctx @ w["wo"].T + w["bo"], w["ln1"])
            h = self._gelu(x @ w["w1"].T + w["b1"])
            x = self._ln(x + h @ w["w2"].T + w["b2"], w["ln2"])
        return x[:, 0]

    @torch.no_grad()
    def head(self, cls):
        cls = torch.as_tensor(np.asarray(cls), dtype=self.dtype)
        return (torch.tanh(cls @ self.wp.T + self.bp) @ self.wc.T + self.bc).numpy()

    def logits(self, ids, types, mask):
        """-> [B, n_labels] numpy in self.dtype."""
        return self.head(self.cls_states(ids, types, mask))


def head_reference(cls, head_sd, dtype):
    """logits of the head alone on rows cls [B, H], torch CPU in `dtype` -> numpy."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    wp, bp, wc, bc = (t(head_sd[n]) for n in HEAD_NAMES)
    with torch.no_grad():
        return (torch.tanh(t(cls) @ wp.T + bp) @ wc.T + bc).numpy()


def oracle(layers, dtype=torch.float64, n_labels=1, seed=0):
    cfg = BertConfig(layers=layers)
    return CrossOracle(cfg, synthetic_state_dict(cfg, seed), synthetic_head_state_dict(cfg, seed, n_labels), dtype)


def pair_batch(seed, B, L, vocab=21128):
    """Seeded (query, document) token pairs: ONE query of 3..11 ids shared by the batch (as a
    reranker sees them), per pair a document of 1 .. L - qn - 3 ids, ids uniform in
    [106, vocab), framed [CLS] q [SEP] d [SEP] with types 0 | 1, ragged right padding (id 0,
    type 0, mask 0).  -> (ids, types, mask) int32 [B, L]."""
    assert L >= 8
    rng = np.random.default_rng([seed, B, L])
    qn = int(rng.integers(3, min(11, L - 4) + 1))
    q = rng.integers(106, vocab, qn)
    ids = np.zeros((B, L), np.int32)
    types = np.zeros((B, L), np.int32)
    mask = np.zeros((B, L), np.int32)
    for b in range(B):
        dn = int(rng.integers(1, L - qn - 3 + 1))
        seq = [CLS] + q.tolist() + [SEP] + rng.integers(106, vocab, dn).tolist() + [SEP]
        ids[b, :len(seq)] = seq
        types[b, qn + 2:len(seq)] = 1
        mask[b, :len(seq)] = 1
    return ids, types, mask


def min_gap(logits):
    """Smallest gap between neighbouring values of the ranked column (inf for one row)."""
    v = np.sort(np.asarray(logits, dtype=np.float64).reshape(-1))
    return float(np.diff(v).min()) if v.size > 1 else float("inf")


def load_golden():
    return np.load(os.path.join(GOLDEN, "cross_encoder_golden.npz"))


def rank_key(layers, B, L):
    return "rank_l%d_b%d_L%d" % (layers, B, L)


def ranking_case(layers, B, L, gold=None):
    """(ids, types, mask, float64 logits [B, 1]) of a ranking case: the generator at the seed the
    golden script found (smallest float64 gap >= MIN_GAP) and the float64 restatement's logits it
    recorded (tests/test_cross_encoder_cases.py recomputes them)."""
    gold = load_golden() if gold is None else gold
    k = rank_key(layers, B, L)
    ids, types, mask = pair_batch(int(gold[k + "_seed"]), B, L)
    return ids, types, mask, np.asarray(gold[k + "_logits64"], dtype=np.float64)
