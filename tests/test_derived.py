"""derived.py: the one cache and invalidation rule for everything built from
an operand's values.  CPU only: CPU tensors carry version counters, and a
plain object with a ``val`` tensor stands in for a CSR."""
import threading

import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import GCN, derived, record
from graph_convolutional_networks_for_text_classification_amd.sparse import CSR


class _Op:
    """Stand-in for a CSR: its values are ``val``."""

    def __init__(self, n=4):
        self.val = torch.zeros(n)


class _Value:
    def __init__(self, pinned=False):
        self.pinned = pinned


class _Builder:
    def __init__(self, make=_Value):
        self.calls, self.make = 0, make

    def __call__(self, *args):
        self.calls += 1
        return self.make(*args)


def test_stamp_follows_in_place_changes_of_every_part():
    t, op = torch.zeros(3), _Op()
    coo = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.tensor([1.0, 2.0]), (2, 2)).coalesce()
    csr = coo.to_sparse_csr()
    for o, bump in ((t, lambda: t.add_(1)), (op, lambda: op.val.mul_(2)), (coo, lambda: coo._values().add_(1)),
                    (coo, lambda: coo._indices().zero_()), (csr, lambda: csr.values().add_(1)),
                    (csr, lambda: csr.col_indices().zero_())):
        held = derived.parts(o)
        before = derived.stamp(o)
        assert before == derived.stamp(o) == derived.stamp(of=held)
        bump()
        assert derived.stamp(o) != before and derived.stamp(of=held) == derived.stamp(o)
    both = derived.parts(t, op, coo)
    assert both[0] is t and both[1] is op.val and len(both) == 4
    assert derived.stamp(t, op) == derived.stamp(t) + derived.stamp(op)
    # an operand known by its storage, not held as an object: the data pointers too
    assert derived.stamp(t, storage=True) == derived.stamp(t, storage=True) != derived.stamp(t.clone(), storage=True)


def test_hit_returns_the_same_object_and_builds_once():
    c, a, x, build = derived.Cache(4), _Op(), torch.zeros(3), _Builder()
    v = c.get("k", (a, x), build)
    assert c.get("k", (a, x), build) is v and build.calls == 1
    assert c.values() == [v] and c.items() == [("k", v)] and len(c.values()) == 1


def test_builder_gets_its_arguments():
    c, a = derived.Cache(), _Op()
    assert c.get((1, 2), (a,), lambda p, q: (p, q), 1, 2) == (1, 2)


def test_in_place_change_of_any_source_rebuilds():
    c, a, x, build = derived.Cache(4), _Op(), torch.zeros(3), _Builder()
    v = c.get("k", (a, x), build)
    x.add_(1)
    w = c.get("k", (a, x), build)
    assert w is not v and build.calls == 2 and c.get("k", (a, x), build) is w
    a.val.mul_(0.5)
    assert c.get("k", (a, x), build) is not w and build.calls == 3 and len(c.values()) == 1


def test_equal_key_with_another_source_object_rebuilds():
    c, a, build = derived.Cache(4), _Op(), _Builder()
    x, y = torch.zeros(3), torch.zeros(3)
    v = c.get("k", (a, x), build)
    assert c.get("k", (a, y), build) is not v and build.calls == 2
    assert c.get("k", (_Op(), y), build) is not v and build.calls == 3


def test_entry_holds_its_sources():
    import weakref
    c, a = derived.Cache(4), _Op()
    x = torch.zeros(3)
    ref = weakref.ref(x)
    c.get(id(x), (a, x), _Builder())
    del x
    assert ref() is not None   # (so the id in the key cannot be recycled while cached)


def test_capacity_evicts_the_oldest_unpinned_entry_never_a_pinned_one():
    derived.release_pinned()
    c, a = derived.Cache(3), _Op()
    vals = [c.get(i, (a,), _Value, i == 0) for i in range(3)]   # entry 0 is pinned
    c.get(3, (a,), _Value)
    assert [k for k, _ in c.items()] == [0, 2, 3]               # 1 was the oldest unpinned
    c.get(4, (a,), _Value)
    assert [k for k, _ in c.items()] == [0, 3, 4] and c.values()[0] is vals[0]
    for v in c.values():
        v.pinned = True
    c.get(5, (a,), _Value)                                      # nothing to evict: the cache grows
    assert [k for k, _ in c.items()] == [0, 3, 4, 5]
    assert derived.PINNED == []                                 # eviction never displaced a pinned value


def test_displaced_pinned_value_is_kept_alive_until_release_pinned():
    derived.release_pinned()
    c, a, build = derived.Cache(2), _Op(), _Builder()
    stale = c.get("k", (a,), build)
    stale.pinned = True                 # a graph was captured through it
    a.val.add_(1)
    fresh = c.get("k", (a,), build)
    assert fresh is not stale and derived.PINNED == [stale]
    unpinned = c.get("u", (a,), build)
    a.val.add_(1)
    assert c.get("u", (a,), build) is not unpinned and derived.PINNED == [stale]   # unpinned: just dropped
    fresh.pinned = True
    c.clear()                           # clearing displaces too
    assert len(c.values()) == 0 and derived.PINNED == [stale, fresh]
    assert record._PINNED is derived.PINNED
    assert record.release_pinned() == 2 and derived.PINNED == [] and record.release_pinned() == 0


def test_none_from_a_builder_is_cached():
    c, a, build = derived.Cache(4), _Op(), _Builder(lambda: None)
    assert c.get("k", (a,), build) is None and c.get("k", (a,), build) is None and build.calls == 1


def test_clear_forces_a_rebuild():
    c, a, build = derived.Cache(4), _Op(), _Builder()
    v = c.get("k", (a,), build)
    c.clear()
    assert c.get("k", (a,), build) is not v and build.calls == 2


def test_namedtuple_keys_are_found_by_plain_tuples():
    c, a, build = derived.Cache(4, record.RecordKey, record.Cached), _Op(), _Builder()
    key = ("fwd", 1, 200, 8, 0, "auto", True, True, True, False)
    v = c.get(key, (a,), build)
    assert c.get(key, (a,), build) is v and build.calls == 1
    (k, got), = c.items()
    assert k.tag == "fwd" and k.F == 200 and type(k) is record.RecordKey
    # the record cache shows its entries as Cached: what readers of adj._records take apart
    assert got.rec is v and got[2] is v and got.srcs == (a,) and c.values()[0].rec is v


def test_cache_of_makes_one_cache_per_owner_and_name():
    a = _Op()
    c = derived.cache_of(a, "_things", 4)
    assert derived.cache_of(a, "_things", 4) is c and a._things is c and c.capacity == 4
    assert derived.cache_of(a, "_others") is not c


def test_eight_threads_on_one_key_build_once():
    c, a, barrier = derived.Cache(4), _Op(), threading.Barrier(8)
    calls, got = [], []

    def build():
        calls.append(1)
        return _Value()

    def work():
        barrier.wait()
        got.append(c.get("k", (a,), build))

    ts = [threading.Thread(target=work) for _ in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert len(calls) == 1 and len(got) == 8 and all(g is got[0] for g in got)


def test_a_builder_may_use_its_own_cache():
    c, a = derived.Cache(4), _Op()
    v = c.get("outer", (a,), lambda: c.get("inner", (a,), _Value))
    assert [k for k, _ in c.items()] == ["inner", "outer"] and c.values() == [v, v]


def _cpu_csr(n, nnz_per_row=1):
    rp = torch.arange(0, n * nnz_per_row + 1, nnz_per_row, dtype=torch.int32)
    ci = torch.arange(n * nnz_per_row, dtype=torch.int32) % n
    return CSR(rp, ci, torch.ones(n * nnz_per_row), (n, n))


def test_gcn_operands_are_rederived_when_a_csr_operand_changes_in_place():
    """GCN.forward's memo of the previous call's operands: a CSR passed as x or
    adj whose values change in place is noticed (on the CPU: a sparse X below
    the dense-operand fill runs no kernel to become an Operand)."""
    m = GCN(nfeat=40, nhid=8, nclass=3, dropout=0.5)
    x, adj = _cpu_csr(40), _cpu_csr(40)
    xop, a = m._operands(x, adj)
    assert a is adj and xop.csr is x
    assert m._operands(x, adj)[0] is xop
    x.val.mul_(0.5)
    xop2 = m._operands(x, adj)[0]
    assert xop2 is not xop and m._operands(x, adj)[0] is xop2
    adj.val.mul_(0.5)
    assert m._operands(x, adj)[0] is not xop2
    assert m._operands(_cpu_csr(40), adj)[0].csr is not x
