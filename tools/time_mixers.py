"""Time TDLearner.train with the transformer, QMIX, VDN and QPLEX (dmaq) mixers.

    python tools/time_mixers.py [--shapes headline,reference-bf16,reference-fp32]
                                [--kinds transformer,qmix,vdn[,dmaq]] [--updates 20] [--warmup 5]

Device events around each update, warm-up first, the variants alternating in one
process (every variant sees the same clocks and the same neighbours), medians printed
as one JSON line per shape.  With one kind and one shape it is the workload of a
`rocprofv3 --kernel-trace --stats` run (profiles/mixers/).
"""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {  # name: (AGVs, episodes, steps, precision)
    "headline": (8, 1024, 60, "bf16"),
    "reference-bf16": (16, 32, 150, "bf16"),
    "reference-fp32": (16, 32, 150, "fp32"),
}


def learner_of(kind, A, precision):
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import TransformerAgent, make_mixer
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(0)
    args = make_args(A, mixer=kind)
    return TDLearner(TransformerAgent(None, args).cuda(), make_mixer(args).cuda(), precision=precision,
                     priorities_to_cpu=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--kinds", default="transformer,qmix,vdn",
                    help="comma-separated args.mixer names: transformer, qmix, vdn, dmaq (= qplex)")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from t2omca_amd.synthetic import make_batch
    kinds = a.kinds.split(",")
    for name in a.shapes.split(","):
        A, B, T, precision = SHAPES[name]
        batch, w = make_batch(B, T, A, seed=1)
        learners = {k: learner_of(k, A, precision) for k in kinds}
        ms = {k: [] for k in kinds}
        for i in range(a.warmup + a.updates):
            for k in kinds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                learners[k].train(batch, 0, i, per_weight=w)
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        out = {"shape": name, "agvs": A, "episodes": B, "steps": T, "precision": precision, "updates": a.updates,
               "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
               "min_ms": {k: round(min(v), 4) for k, v in ms.items()}}
        if "qmix" in ms and "transformer" in ms:
            out["qmix_faster_than_transformer"] = out["median_ms"]["qmix"] < out["median_ms"]["transformer"]
        for k in ("dmaq", "qplex"):
            if k in ms and "transformer" in ms:
                out[k + "_faster_than_transformer"] = out["median_ms"][k] < out["median_ms"]["transformer"]
        print(json.dumps(out), flush=True)
        del learners, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
