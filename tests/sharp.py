"""Sharp-softmax inputs for the oracle comparisons (test helpers; CPU code only).

Default initialisation and N(0, 1) inputs leave the attention scores within about
|s| < 2, where the softmax is close to uniform and neither the max
subtraction, the running-max rescale of the chunked agent, the -inf padding masks nor
the BPTT's recomputed probabilities can go wrong.  Multiplying every
attention.tokeys.weight and attention.toqueries.weight by s scales the scores by s²
while the fp64 oracle stays exact, so the same references reach the regime a trained
policy runs in.  Here:

    sharpen / sharpen_   the scaled parameters (a state-dict-style dict / modules in place)
    softmax_stats        what the softmax rows of a case look like, from the fp64 oracle
    fp32_fit             how far float32 (or bf16-operand) arithmetic alone is from fp64
                         on a case, in the kernels' folded association

The GPU files assert nothing about sharpness themselves: tests/test_sharp_inputs.py
asserts, without a device, that each of their cases is sharp enough to bite and that
rounding alone stays clear of the bars they apply.
"""
import collections
import contextlib

import torch
import torch.nn.functional as F

from oracle import ref_model
from tests.gpu_util import normwise
from tests.grad_blocks import Bf16Operands

SHARP_KEYS = ("attention.tokeys.weight", "attention.toqueries.weight")
AGENT_CHUNK = 8   # t2o_agent_block_ch.hpp AG_CHUNK: entities per streamed chunk (key 0 is the hidden token)
KEY_TILE = 16     # t2o_mixer_block.hpp key_mask: keys per score tile


def sharpen(params, s):
    """A copy of a state-dict-style dict with every attention.tokeys.weight and
    attention.toqueries.weight multiplied by s (the scores scale by s²)."""
    hit = [k for k in params if k.endswith(SHARP_KEYS)]
    assert hit, "no attention.tokeys / toqueries weights among the parameters"
    return {k: (v * s if k in hit else v.clone()) for k, v in params.items()}


def sharpen_(s):
    """The in-place form: a callable that scales the same weights of every module it is
    given, under torch.no_grad() (tests/test_gpu_generic._td's `prepare`)."""
    def prepare(*modules):
        with torch.no_grad():
            for mod in modules:
                hit = [p for k, p in mod.named_parameters() if k.endswith(SHARP_KEYS)]
                assert hit, "no attention.tokeys / toqueries weights in the module"
                for p in hit:
                    p.mul_(s)
    return prepare


class _RecordSoftmax:
    """While entered, oracle.ref_model.mha is a restatement of itself that also records
    the scores of the query rows whose output is consumed (the way
    grad_blocks.Bf16Operands(fold=True) swaps it; torch.nn.functional is untouched).
    Networks are told apart by their token counts: n_ent + 1 keys is an agent (consumed
    query: token 0, the hidden state), n_ent + n_agents + 3 a mixer (the last
    n_agents + 3 tokens)."""

    def __init__(self, n_agents, n_ent=None):
        n_ent = n_agents if n_ent is None else n_ent
        self.rows = {n_ent + 1: ("agent", slice(0, 1)), n_ent + n_agents + 3: ("mixer", slice(-n_agents - 3, None))}
        self.scores = collections.defaultdict(list)

    def __enter__(self):
        self._mha, ref_model.mha = ref_model.mha, self._recording_mha
        return self

    def __exit__(self, *exc):
        ref_model.mha = self._mha

    def _recording_mha(self, p, pre, q, k, heads):
        b, t_q, e = q.shape
        t_k = k.shape[1]
        keys = F.linear(k, p[pre + "tokeys.weight"]).view(b, t_k, heads, e).transpose(1, 2) / e ** 0.25
        values = F.linear(k, p[pre + "tovalues.weight"]).view(b, t_k, heads, e).transpose(1, 2)
        queries = F.linear(q, p[pre + "toqueries.weight"]).view(b, t_q, heads, e).transpose(1, 2) / e ** 0.25
        dot = torch.matmul(queries, keys.transpose(-1, -2))  # [b, h, t_q, t_k]
        net, rows = self.rows[t_k]
        self.scores[net].append(dot.detach()[:, :, rows].reshape(-1, t_k))
        out = torch.matmul(F.softmax(dot, dim=-1), values).transpose(1, 2).reshape(b, t_q, heads * e)
        return F.linear(out, p[pre + "unifyheads.weight"], p[pre + "unifyheads.bias"])


def softmax_stats(run, n_agents, n_ent=None):
    """run() evaluates the fp64 oracle on a case; every softmax row of a consumed query
    is recorded.  Returns per network ("agent" / "mixer") a dict: spread = the largest
    (row max - row min) over finite scores, max_abs = the largest |score|, max = the
    largest score, min_rowmax = the smallest row maximum, maxprob = the mean
    max-probability, hist = how often the argmax fell on each key position."""
    with _RecordSoftmax(n_agents, n_ent) as rec, torch.no_grad():
        run()
    out = {}
    for net, rows in rec.scores.items():
        s = torch.cat(rows).double()
        assert bool(torch.isfinite(s).all())
        rowmax = s.max(1).values
        out[net] = dict(spread=float((rowmax - s.min(1).values).max()), max_abs=float(s.abs().max()),
                        max=float(s.max()), min_rowmax=float(rowmax.min()),
                        maxprob=float(F.softmax(s, 1).max(1).values.mean()),
                        hist=torch.bincount(s.argmax(1), minlength=s.shape[1]), rows=s.shape[0])
    return out


def agent_chunks_hit(hist):
    """(hidden token, first chunk, last chunk): argmax counts of an agent's histogram
    (key 0 = hidden state, then the entities in chunks of AGENT_CHUNK; the last chunk
    is the partial one when the entity count is no multiple)."""
    ne = hist.numel() - 1
    last0 = 1 + AGENT_CHUNK * ((ne - 1) // AGENT_CHUNK)
    return int(hist[0]), int(hist[1:1 + AGENT_CHUNK].sum()), int(hist[last0:].sum())


def mixer_tiles_hit(hist):
    """(first key tile, last key tile): argmax counts of a mixer's histogram."""
    last0 = KEY_TILE * ((hist.numel() - 1) // KEY_TILE)
    return int(hist[:KEY_TILE].sum()), int(hist[last0:].sum())


@contextlib.contextmanager
def one_thread():
    """float32 sums depend on how they are split over threads; the fitness figures are taken
    on one thread so that they do not move with the thread count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def fp32_fit(evaluate, ref, precision="fp32", attention=True):
    """evaluate(dtype) -> dict of tensors (the case's checked quantities, computed by
    the oracle in dtype).  Runs it in float32 with the attention in the kernels' folded
    association and nothing rounded (precision "fp32"), or in fp64 with bf16 matmul
    operands (precision "bf16": Bf16Operands(fold=True)), and returns the normwise
    error of each quantity against `ref` (the plain fp64 evaluation).  attention=False:
    a model without attention (the flat mixers, the GRU agent), plainly in float32."""
    if not attention:
        assert precision == "fp32"
        with one_thread():
            got = evaluate(torch.float32)
        return {k: normwise(v, ref[k]) for k, v in got.items()}
    if precision == "fp32":
        mode, dtype = Bf16Operands(rounding=False, fold=True), torch.float32
    else:
        mode, dtype = Bf16Operands(fold=True), torch.float64
    with mode, one_thread():
        got = evaluate(dtype)
    assert mode.calls > 0
    return {k: normwise(v, ref[k]) for k, v in got.items()}
