"""bench.py's command line: a plain run times --steps steps of the headline alone and leaves
what --full measures null; --dump-outputs writes the last timed step's arrays, which are the
exact top-k of the dumped embeddings over the seeded corpus (float64 oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.flat import check_topk, exact_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = [sys.executable, os.path.join(ROOT, "bench.py")]


def test_bench_rejects_zero_steps_and_lists_the_options():
    r = subprocess.run(BENCH + ["--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
    h = subprocess.run(BENCH + ["--help"], capture_output=True, text=True, timeout=120)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_outputs(require_gpu, tmp_path):
    import torch
    from mediquery_hip import synth
    n, B, K, steps = 20000, 64, 5, 3
    d = tmp_path / "dump"
    r = subprocess.run(BENCH + ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--corpus-rows", str(n),
                                "--batch", str(B), "--layers", "2", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["unit"] == "queries/s" and out["higher_is_better"] is True
    # value = queries / time of the same steps (ms_per_step is printed rounded to 1e-3 ms)
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - B / out["ms_per_step"] * 1e3) <= (6e-4 / out["ms_per_step"]) * out["value"] + 0.01
    assert out["full"] is False
    for key in ("cpu_baseline", "exact_f32_encoder", "f32_direct_search", "split_f32", "config4_sharded",
                "config5_bf16_rerank", "secondary_long_queries", "p50_single_query_ms", "planted_top1_ok"):
        assert out[key] is None, key
    for key in ("exact_k50_batch", "long_query_p50", "config2", "clustered_corpus", "langchain_embed_documents"):
        assert key not in out
    assert sorted(os.listdir(d)) == ["embeddings.npy", "ids.npy", "scores.npy"]
    emb, ids, scores = (np.load(d / (name + ".npy")) for name in ("embeddings", "ids", "scores"))
    assert emb.dtype == np.float32 and emb.shape == (B, 768)
    assert scores.dtype == np.float32 and scores.shape == (B, K)
    assert ids.dtype == np.float64 and ids.shape == (B, K) and (ids == np.floor(ids)).all()
    corpus = synth.corpus_device(n, 768, torch.device("cuda", 0)).cpu().numpy()
    fails = check_topk(ids.astype(np.int64), scores, exact_scores(emb, corpus), K)
    assert not fails, fails[:3]
