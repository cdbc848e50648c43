"""Tensors derived from a parameter, cached against version counters."""


class _Derived(dict):
    """A tensor's cache entries; a copy or pickle of the tensor starts empty."""

    def __deepcopy__(self, memo):
        return _Derived()

    def __reduce__(self):
        return _Derived, ()


def versioned(owner, tag, versions, build, *args):
    """``build(previous, *args)``, rebuilt only when ``versions`` (a tuple of
    ``_version`` counters) differs from the one it was built at; a hit returns
    the very same object. ``previous`` is the stale value (``None`` the first
    time) whose buffers a build can reuse; a module-level ``build`` keeps
    the hit path free of closures.

    The entries hang on the tensor ``owner`` itself, one dict per owner keyed
    by ``tag``: they die with it, nothing outlives a deleted model, and no
    id() can be recycled into a stale hit (docs/KERNELS.md, "Host planning").
    Values must not reference the owner."""
    try:
        cache = owner._ibp_derived
    except AttributeError:
        cache = owner._ibp_derived = _Derived()
    entry = cache.get(tag)
    if entry is not None and entry[0] == versions:
        return entry[1]
    value = build(entry[1] if entry is not None else None, *args)
    cache[tag] = (versions, value)
    return value
