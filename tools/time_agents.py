"""Time TDLearner.train (mixer: qmix) with the transformer agent and with the GRU agent
(agent: rnn), and the GRU agent's kernels one by one.

    python tools/time_agents.py [--shapes large,small] [--updates 20] [--warmup 5] [--kernels]

Device events around each update, warm-up first, the two agents alternating in one
process (both see the same clocks and the same neighbours), medians printed as one JSON
line per shape.  --kernels adds the per-entry-point split of the GRU agent (forward of
both networks, backward of one: device events around each wrapper call, same protocol).
There is no bar on these figures: they are recorded, not asserted.
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {  # name: (AGVs, episodes, steps)
    "large": (8, 1024, 60),
    "small": (16, 32, 150),
}
NA = 5


def learner_of(agent_kind, A):
    from t2omca_amd.learner import TDLearner
    from t2omca_amd.modules import make_agent, make_mixer
    from t2omca_amd.synthetic import make_args
    torch.manual_seed(0)
    args = types.SimpleNamespace(**{**vars(make_args(A, mixer="qmix")), "agent": agent_kind})
    agent = make_agent(9 * A + NA + A, args).cuda()
    return TDLearner(agent, make_mixer(args).cuda(), priorities_to_cpu=False)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernel_split(learner, batch, updates, warmup):
    """Median ms of the GRU agent's forward (both networks) and backward (one) alone."""
    from t2omca_amd import ops
    sh, na = learner.sa, learner.na
    obs, act = batch["obs"], batch["actions"][..., 0]
    B, T1, A, _ = obs.shape
    gch = torch.randn(B, T1 - 1, A, device=obs.device)
    fwd_ms, bwd_ms = [], []
    for i in range(warmup + updates):
        tf, fwd = timed(lambda: ops.rnn_agent_fwd(sh, learner.params[:na], obs, actions=act,
                                                  params_tg=learner.target_params[:na]))
        tb, _ = timed(lambda: ops.rnn_agent_bwd(sh, learner.params[:na], obs, fwd, T=T1 - 1, actions=act, gchosen=gch))
        if i >= warmup:
            fwd_ms.append(tf)
            bwd_ms.append(tb)
    return {"rnn_fwd_two_networks": round(statistics.median(fwd_ms), 4),
            "rnn_bwd_with_weight_gradients": round(statistics.median(bwd_ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--agents", default="transformer,rnn")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    from t2omca_amd.synthetic import make_batch
    kinds = a.agents.split(",")
    for name in a.shapes.split(","):
        A, B, T = SHAPES[name]
        batch, w = make_batch(B, T, A, seed=1)
        learners = {k: learner_of(k, A) for k in kinds}
        ms = {k: [] for k in kinds}
        for i in range(a.warmup + a.updates):
            for k in kinds:
                t, _ = timed(lambda: learners[k].train(batch, 0, i, per_weight=w))
                if i >= a.warmup:
                    ms[k].append(t)
        out = {"shape": name, "agvs": A, "episodes": B, "steps": T, "mixer": "qmix", "precision": "fp32",
               "updates": a.updates, "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
               "min_ms": {k: round(min(v), 4) for k, v in ms.items()}}
        if a.kernels and "rnn" in learners:
            out["rnn_kernels_median_ms"] = kernel_split(learners["rnn"], batch, a.updates, a.warmup)
        print(json.dumps(out), flush=True)
        del learners, batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
