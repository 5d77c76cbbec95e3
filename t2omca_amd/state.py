"""Helpers of the objects' ``state_dict()`` / ``load_state_dict(sd)`` (VecEnv,
RolloutRunner, PrioritizedReplayBuffer, TDLearner; driver.save_run_state).

A saved state is a plain dict of CPU tensors, ints, floats, strings, lists and
dicts with ``"format": 1``, so ``torch.load(weights_only=True)`` keeps it.  A load
copies in place into the object's existing device tensors and raises ValueError,
naming the field, when the saved object was built differently.
"""


def check_fields(who, sd, want):
    """ValueError naming the first field of ``want`` that ``sd`` lacks or holds with
    another value (tuples and lists compare equal: a saved tuple comes back a list)."""
    for k, v in want.items():
        if k not in sd:
            raise ValueError(f"{who} state: field {k!r} is missing")
        got = sd[k]
        if isinstance(v, (tuple, list)):
            v, got = _listed(v), _listed(got)
        if got != v:
            raise ValueError(f"{who} state: {k} is {got!r} in the saved state, {v!r} here")


def _listed(v):
    return [_listed(x) for x in v] if isinstance(v, (tuple, list)) else v


def copy_checked(who, name, dst, src):
    """dst.copy_(src) after checking shape and dtype."""
    if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        raise ValueError(f"{who} state: {name} is {tuple(src.shape)} {src.dtype} in the saved state, "
                         f"{tuple(dst.shape)} {dst.dtype} here")
    dst.copy_(src)
