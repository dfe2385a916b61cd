"""Everything built once from an operand's values and reused -- SpMM plans,
transposes, dense copies, hub factors, A-hat X, launch records -- is kept in a
Cache held on the owning operand, under one rule:

  * an entry is a hit only while every source it was built from IS the same
    object and has the stamp() it had then (an in-place change of a tensor's
    values bumps its version counter, so everything derived from them is
    rebuilt, not only some of it);
  * the entry holds its sources, so an id() cannot be recycled while cached;
  * a miss builds once, under the cache's lock; a builder's None is cached;
  * a full cache evicts its oldest entry that is not pinned.  A value is
    PINNED (its ``pinned`` attribute) once a hipGraph captured while it was in
    use may still point into its buffers, through raw pointers no reference
    count sees;
  * a pinned value displaced from any cache (stale, replaced, cleared) goes on
    the one keep-alive list PINNED, which only release_pinned() drops.

This module is the only place that reads a version counter or a data pointer
to tell whether cached state is still good.
"""
import operator
import threading

import torch


def parts(*operands):
    """The tensors that carry the operands' values, in one flat tuple: a dense
    tensor itself, the index and value tensors of a torch sparse COO / CSR
    tensor, ``val`` of a CSR (whose arrays are set once, never rebound)."""
    out = ()
    for o in operands:
        if not isinstance(o, torch.Tensor):
            out += (o.val,)
        elif o.layout == torch.strided:
            out += (o,)
        elif o.layout == torch.sparse_coo:
            out += (o._indices(), o._values())
        else:
            out += (o.crow_indices(), o.col_indices(), o.values())
    return out


_version, _data_ptr = operator.attrgetter("_version"), torch.Tensor.data_ptr


def stamp(*operands, of=None, storage=False):
    """The value-identity of the operands: the version counter of each of their
    parts, which every in-place change bumps.  Equal stamps of the same objects
    mean unchanged values.  ``of``: parts(*operands) from an earlier call (they
    alias the operands' data), which saves taking them again.  ``storage``:
    with the parts' data pointers, for an operand known by its storage and not
    held as an object (sparse.CACHE)."""
    if of is None:
        of = parts(*operands)
    v = tuple(map(_version, of))
    return v + tuple(map(_data_ptr, of)) if storage else v


PINNED = []   # pinned values displaced from their cache, kept alive until release_pinned()
_pinned_lock = threading.Lock()


def _retire(value):
    if getattr(value, "pinned", False):
        with _pinned_lock:
            if not any(v is value for v in PINNED):
                PINNED.append(value)


def release_pinned():
    """Drop the values kept alive for hipGraphs captured before their operands
    changed (call after those graphs are destroyed; replaying one afterwards
    reads and writes freed memory).  Returns how many were dropped."""
    with _pinned_lock:
        n = len(PINNED)
        PINNED.clear()
    return n


class _Entry:
    __slots__ = ("srcs", "parts", "stamp", "value")

    def __init__(self, srcs, value):
        self.srcs, self.value = srcs, value
        self.parts = parts(*srcs)
        self.stamp = stamp(of=self.parts)


def _holds(e, srcs):
    """Entry `e` was built from the objects `srcs` and all its sources keep their stamps."""
    held = e.srcs
    for i in range(len(srcs)):
        if srcs[i] is not held[i]:
            return False
    return stamp(of=e.parts) == e.stamp


class Cache:
    """key -> value built from source operands; see the module docstring.
    ``capacity``: entries kept (None: no bound); ``key_type``: a namedtuple
    class the stored keys are made of (lookups pass its fields as a plain tuple);
    ``shown_as``: a namedtuple class of (sources, stamp, value) that values()
    and items() show each entry as, instead of the bare value."""

    __slots__ = ("capacity", "key_type", "shown_as", "_d", "_lock")

    def __init__(self, capacity=None, key_type=None, shown_as=None):
        self.capacity, self.key_type, self.shown_as = capacity, key_type, shown_as
        self._d = {}
        self._lock = threading.RLock()   # (a builder may look up the same cache)

    def get(self, key, srcs, build, *args):
        """The value under ``key`` built from the operands ``srcs``:
        ``build(*args)`` on first use and whenever a source has changed."""
        e = self._d.get(key)
        if e is not None and _holds(e, srcs):
            return e.value
        with self._lock:
            e = self._d.get(key)
            if e is not None and _holds(e, srcs):
                return e.value
            return self.put(key, srcs, build(*args))

    def put(self, key, srcs, value):
        """File ``value`` as built from ``srcs`` under ``key``; returns it.  (Sources
        past those a lookup names are held to their stamps all the same.)"""
        with self._lock:
            d = self._d
            old = d.pop(key, None)
            if old is not None and old.value is not value:
                _retire(old.value)
            while self.capacity is not None and len(d) >= self.capacity:
                victim = next((k for k, e in d.items() if not getattr(e.value, "pinned", False)), None)
                if victim is None:
                    break
                del d[victim]
            d[self.key_type(*key) if self.key_type is not None else key] = _Entry(tuple(srcs), value)
        return value

    def clear(self):
        with self._lock:
            for e in self._d.values():
                _retire(e.value)
            self._d.clear()

    def items(self):
        """[(key, value)], oldest first."""
        show = self.shown_as
        return [(k, e.value if show is None else show(e.srcs, e.stamp, e.value)) for k, e in list(self._d.items())]

    def values(self):
        return [v for _, v in self.items()]


def cache_of(owner, name, *how):
    """The Cache kept on ``owner`` as attribute ``name``, made on first use as Cache(*how)."""
    c = owner.__dict__.get(name)
    if c is None:
        c = owner.__dict__.setdefault(name, Cache(*how))   # (atomic: two threads get one cache)
    return c
