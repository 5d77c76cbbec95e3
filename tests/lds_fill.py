"""Stale-LDS sweep helper (test helper, no tests): run a launch after LDS was filled
with each of three words and require that the fill never reaches an output.

A kernel that reads an LDS word it did not write gets whatever the previous workgroup
on that CU left there.  ops.lds_fill(word) leaves `word` in every 32-bit word of every
CU's LDS (tests/test_gpu_stale_lds.py measures that it does); the launch under test
then runs, where the case can arrange it, on fewer workgroups than the device has CUs,
so each of them is the first on its CU after the fill (tests/test_gpu_stale_lds.py lists
the launches for which it cannot).

  0x00000000  the baseline run.
  0xFFFFFFFF  NaN as fp32 and in both bf16 halves: any arithmetic use of a stale word
              becomes NaN.
  0x7F7F7F7F  about 3.4e38 as fp32 and in both bf16 halves: finite and positive, so it
              survives what swallows a NaN (v_max_f32 returns its non-NaN operand, so
              fmaxf and a ReLU over a stale NaN hide the read).
"""
import torch

from tests.gpu_util import normwise

ZERO, NAN, HUGE = 0x00000000, 0xFFFFFFFF, 0x7F7F7F7F
PATTERNS = (ZERO, NAN, HUGE)
# the project's summation-order bar (tests/test_gpu_fullgrid.py GRAD_SUM_BAR): outputs
# summed with float atomics in varying order are held to it instead of bit equality
SUM_BAR = 1e-6


_current = [None]


def refill():
    """The pattern of the run in progress once more: a case of several launches calls this
    before each launch after the first, so that each of them starts from the fill."""
    from t2omca_amd import ops
    assert _current[0] is not None, "refill() outside under_each_fill"
    torch.cuda.synchronize()
    ops.lds_fill(_current[0])


def _named(outs):
    if isinstance(outs, dict):
        return list(outs.items())
    return [(str(i), t) for i, t in enumerate(outs)]


def under_each_fill(fn, *, sum_order=(), before=None, tag=""):
    """fn() under each fill pattern.  For every pattern: `before()` if given (restores
    state a run consumed; its own launches precede the fill), synchronise,
    ops.lds_fill(pattern), fn() (which calls refill() before each further launch
    of its own).  fn() allocates nothing but torch.empty outputs
    between the fill and its launches, launches nothing that is not under test, and
    returns clones of every output (a dict or a sequence of tensors; None entries are
    dropped).  Asserts that every floating-point output is finite under all three
    patterns, and that the outputs under the NaN and the huge fill are torch.equal to
    the zero-fill baseline; outputs named in `sum_order` (float atomics in varying
    order) are held to SUM_BAR normwise instead.  Returns the baseline outputs."""
    from t2omca_amd import ops
    runs = {}
    for pat in PATTERNS:
        if before is not None:
            before()
        torch.cuda.synchronize()
        ops.lds_fill(pat)
        _current[0] = pat
        try:
            outs = fn()
        finally:
            _current[0] = None
        torch.cuda.synchronize()
        runs[pat] = [(k, t) for k, t in _named(outs) if t is not None]
    base = runs[ZERO]
    assert base, "the case returned no output"
    bad = []
    for pat in PATTERNS:
        assert [k for k, _ in runs[pat]] == [k for k, _ in base]
        for (k, t), (_, b) in zip(runs[pat], base):
            if t.is_floating_point() and not bool(torch.isfinite(t).all()):
                bad.append(f"{tag} output {k} under fill {pat:#010x}: "
                           f"{int((~torch.isfinite(t)).sum())} of {t.numel()} non-finite")
                continue
            if pat == ZERO:
                continue
            if k in sum_order:
                err = normwise(t, b)
                if not err < SUM_BAR:
                    bad.append(f"{tag} output {k} under fill {pat:#010x}: {err:.2e} normwise from the zero fill's")
            elif not torch.equal(t, b):
                bad.append(f"{tag} output {k} under fill {pat:#010x}: {int((t != b).sum())} of {t.numel()} "
                           f"elements differ from the zero fill's, normwise {normwise(t, b):.2e}")
    assert not bad, "\n".join(bad)
    return dict(base)
