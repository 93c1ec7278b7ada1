"""Accuracy record of MQ_ENC_OPT_LN_FOLD: max |err| of the split-f32 encoder against a float64
restatement of the oracle, fold off and fold on, at the bench shape (12-layer BERT-base, B =
256, L = 32, the bench's token ids).  Run on the GPU box from the repo root:

  python tools/ln_fold_accuracy.py [--out profiles/ln_fold/accuracy.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mediquery-rag_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mediquery_hip import _lib, synth  # noqa: E402
from mediquery_hip.config import DMETA_BASE  # noqa: E402
from mediquery_hip.native import Encoder  # noqa: E402
from mediquery_hip.weights import synthetic_state_dict  # noqa: E402
from oracle.encoder import OracleEncoder  # noqa: E402


def oracle_f64(cfg, ids, mask):
    """The oracle's arithmetic with every tensor in float64."""
    o = OracleEncoder(cfg, synthetic_state_dict(cfg, 0))
    d = lambda t: t.double()
    o.word, o.pos, o.typ, o.eln = d(o.word), d(o.pos), d(o.typ), tuple(d(t) for t in o.eln)
    o.layers = [{k: (tuple(d(t) for t in v) if isinstance(v, tuple) else d(v)) for k, v in w.items()}
                for w in o.layers]
    h = o.hidden_states(ids, mask)
    e = h[:, 0]
    return (e / e.norm(dim=-1, keepdim=True)).numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = DMETA_BASE
    ids, mask = synth.token_batch(256, 32)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref = oracle_f64(cfg, ids, mask)
    enc = Encoder(cfg)
    enc.set_precision(_lib.MQ_DTYPE_F32X6)
    lines = []
    errs = {}
    for fold in (0, 1):
        enc.set_option("ln_fold", fold)
        got = enc.embed(ids, mask).astype(np.float64)
        err = np.abs(got - ref)
        cos = (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)
        errs[fold] = err.max()
        lines.append("ln_fold=%d  max|err| %.4g  mean|err| %.4g  min cos %.12f" % (fold, err.max(), err.mean(), cos.min()))
    lines.append("fold on / fold off max|err| ratio %.3f (allowed: 2)" % (errs[1] / errs[0]))
    text = ("split-f32 encoder vs float64 oracle, 12 layers, B = 256, L = 32, CLS pooling\n" + "\n".join(lines) + "\n")
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
