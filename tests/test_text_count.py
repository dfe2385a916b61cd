"""TextCounter on the GPU (csrc/text_count.hip: gcnk_text_count, gcnk_text_emit) against tests/text_ref.py's
pure-Python restatement, itself pinned on the CPU (test_text_ref.py) to sklearn's CountVectorizer.transform, and
against sklearn's recorded transform of the fixture.  The result is integers, so every comparison is equality of
all three arrays, dtypes included.  Expected values never come from the code under test."""
import numpy as np
import pytest
import torch

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import TextCounter, TopicInferencer, doc_term, fit_topics

import text_ref as R
from lda_gpu import DEV, bits as _bits, dev as _dev

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    """The counter's three device arrays against three host arrays (indptr, indices, counts)."""
    ip, ix, ct = got
    assert ip.dtype == torch.int32 and ix.dtype == torch.int32 and ct.dtype == torch.float64, what
    assert all(t.device == torch.device(DEV) and t.dim() == 1 and t.is_contiguous() for t in got), what
    for name, t, w in zip(("indptr", "indices", "counts"), got, want):
        w = torch.from_numpy(np.ascontiguousarray(w, dtype={"counts": np.float64}.get(name, np.int32)))
        assert torch.equal(t.cpu(), w), (what, name, t.cpu()[:40], w[:40])


def _check(counter, texts, words, what=""):
    want = R.transform(texts, words)
    got = counter(texts)
    _same(got, want, what)
    return got, want


@pytest.fixture(scope="module")
def gold():
    return R.golden()


@pytest.fixture(scope="module")
def adv():
    return TextCounter(R.ADVERSARIAL_WORDS, DEV)


def test_fixture_both_ways_and_twice(gold):
    counter = TextCounter(gold["words"], DEV)
    want = (gold["indptr"], gold["indices"], gold["data"])              # sklearn's recorded transform
    one = counter(gold["texts"])
    _same(one, want, "counter(texts)")
    data, offsets = counter.pack(gold["texts"])
    assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and data.device == offsets.device == one[0].device
    assert data.cpu().numpy().tobytes() == gold["text_bytes"].tobytes()
    assert np.array_equal(offsets.cpu().numpy(), gold["text_offsets"])
    two = counter.count(data, offsets)
    _same(two, want, "pack + count")
    again = counter(gold["texts"])
    for a, b in zip(one, again):
        assert torch.equal(_bits(a) if a.dtype == torch.float64 else a, _bits(b) if b.dtype == torch.float64 else b)
    # from a str -> id mapping too, and a part of the batch alone
    mapped = TextCounter({w: i for i, w in enumerate(gold["words"])}, DEV)
    _same(mapped(gold["texts"][200:]), R.transform(gold["texts"][200:], gold["words"]), "the unseen documents alone")


def test_from_sklearn_counts_what_transform_counts(gold):
    fe = pytest.importorskip("sklearn.feature_extraction.text")
    vec = fe.CountVectorizer(token_pattern=r"\S+", lowercase=False).fit(gold["texts"][:200])
    counter = TextCounter.from_sklearn(vec, DEV)
    for texts in (gold["texts"], R.ADVERSARIAL_TEXTS):
        host = doc_term(vec.transform(texts), DEV)
        got = counter(texts)
        assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(got, host))


def test_adversarial_texts(adv):
    got, want = _check(adv, R.ADVERSARIAL_TEXTS, R.ADVERSARIAL_WORDS, "the whole list")
    assert want[0][-1] > 60
    for i, t in enumerate(R.ADVERSARIAL_TEXTS[:6] + R.ADVERSARIAL_TEXTS[-12:]):      # and alone: B = 1
        _check(adv, [t], R.ADVERSARIAL_WORDS, f"text {i} alone")


def test_piece_boundaries(adv):
    texts = ["x" * i + " oil " + "y" * i + "price" for i in range(131)]
    got, want = _check(adv, texts, R.ADVERSARIAL_WORDS)
    # "y" * 0 + "price" counts price; with i > 0 the token is y..yprice: only oil is left
    assert want[0].tolist() == [0, 2] + list(range(3, 133)) and got[0][-1].item() == 132
    _check(adv, list(reversed(texts)), R.ADVERSARIAL_WORDS, "reversed")
    texts = ["x" * i + " price " + "oil" + " " * i + "a" for i in range(131)]
    _check(adv, texts, R.ADVERSARIAL_WORDS, "white-space runs across pieces")


def test_adjacent_documents_do_not_merge(adv):
    texts = ["crude oil", "price oil"]
    data, offsets = adv.pack(texts)
    assert data.cpu().numpy().tobytes() == b"crude oilprice oil" and offsets.tolist() == [0, 9, 18]
    got, _ = _check(adv, texts, R.ADVERSARIAL_WORDS)
    merged = TextCounter(["oilprice", "oil", "price"], DEV)
    ip, ix, ct = merged(["oil", "price"])                    # two rows, one entry each
    assert ip.tolist() == [0, 1, 2] and ix.tolist() == [1, 2] and ct.tolist() == [1.0, 1.0]
    ip, ix, ct = merged.count(_dev(np.array(list(b"oilprice"), np.uint8)), _dev(np.array([0, 8], np.int64)))
    assert ip.tolist() == [0, 1] and ix.tolist() == [0] and ct.tolist() == [1.0]     # one document: one token
    _check(merged, ["a oil", "price", "oil", "price b", "", "oil", "", "price"], ["oilprice", "oil", "price"])


def test_long_document(gold):
    rng = np.random.RandomState(7)
    words = gold["words"]
    pick = rng.choice(len(words), 300, replace=False)
    long_doc = " ".join(words[pick[j]] for j in rng.randint(0, 300, 20000))
    counter = TextCounter(words, DEV)
    got, want = _check(counter, [long_doc], words)
    assert want[0].tolist() == [0, 300] and want[2].sum() == 20000.0
    _check(counter, [gold["texts"][0], long_doc, "", gold["texts"][1], long_doc[:70001]], words, "among short ones")


def test_repeated_word(adv):
    ip, ix, ct = adv([" ".join(["price"] * 70000)])
    assert ip.tolist() == [0, 1] and ix.tolist() == [1] and ct.tolist() == [70000.0]
    ip, ix, ct = adv(["oil", "\n".join(["price"] * 70000) + "\toil", "price"])
    assert ip.tolist() == [0, 1, 3, 4] and ix.tolist() == [0, 0, 1, 1] and ct.tolist() == [1.0, 1.0, 70000.0, 1.0]


def test_sizes(adv):
    ip, ix, ct = adv([])
    assert ip.tolist() == [0] and ip.dtype == torch.int32
    assert ix.numel() == 0 and ct.numel() == 0 and ix.dtype == torch.int32 and ct.dtype == torch.float64
    _check(adv, [], R.ADVERSARIAL_WORDS, "B = 0")
    for texts in (["oil"], ["x"], [""], ["", "", ""], ["   ", "\t", ""], ["oil", ""], ["", "oil"],
                  ["", "", "oil price", "", "price oil oil", "a", "", ""]):
        _check(adv, texts, R.ADVERSARIAL_WORDS, repr(texts))
    one = TextCounter(["x"], DEV)                                         # the least vocabulary
    _check(one, ["x", "xx x", "", "y x x"], ["x"])


def test_equal_hashes_are_told_apart_by_their_bytes():
    a, b = R.colliding_pair()
    assert a != b and R.fnv1a(a.encode()) == R.fnv1a(b.encode())
    only_a = TextCounter([a, "oil"], DEV)
    ip, ix, ct = only_a([f"{b} {b} oil"])
    assert ip.tolist() == [0, 1] and ix.tolist() == [1] and ct.tolist() == [1.0]      # b is not counted as a
    _check(only_a, [f"{b} oil {a} {b}", b, a], [a, "oil"])
    both = TextCounter([a, "oil", b], DEV)
    ip, ix, ct = both([f"{b} {a} {b} oil {b}"])
    assert ip.tolist() == [0, 3] and ix.tolist() == [0, 1, 2] and ct.tolist() == [1.0, 1.0, 3.0]
    _check(both, [f"{b} oil {a} {b}", b, a], [a, "oil", b])


def test_plumbing_into_the_topic_model(gold):
    words, texts = gold["words"], gold["texts"]
    counter = TextCounter(words, DEV)
    got = counter(texts)
    try:
        from sklearn.feature_extraction.text import CountVectorizer
        host = doc_term(CountVectorizer(vocabulary=words, token_pattern=r"\S+", lowercase=False).transform(texts), DEV)
    except ImportError:
        host = (_dev(gold["indptr"]), _dev(gold["indices"]), _dev(gold["data"].astype(np.float64)))
    K, V = 8, len(words)
    lam = _dev(np.random.RandomState(3).gamma(100.0, 0.01, (K, V)))
    inf = TopicInferencer.from_components(lam, 1.0 / K)
    x, a = inf.scorer_operands(*got, 0.02)
    xh, ah = inf.scorer_operands(*host, 0.02)
    assert torch.equal(_bits(x), _bits(xh)) and torch.equal(_bits(a), _bits(ah)) and tuple(x.shape) == (300, K)
    fit = fit_topics(*got, V, num_topics=4, max_iter=2)
    ref = fit_topics(*host, V, num_topics=4, max_iter=2)
    assert torch.equal(_bits(fit.components), _bits(ref.components))


def test_cpu_tensors_and_wrong_operands_are_refused(adv):
    data, offsets = adv.pack(["oil price"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        adv.count(data.cpu(), offsets)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        adv.count(data, offsets.cpu())
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        adv.count(np.frombuffer(b"oil", np.uint8), offsets)
    with pytest.raises(RuntimeError, match="uint8"):
        adv.count(data.to(torch.int32), offsets)
    with pytest.raises(RuntimeError, match="int64"):
        adv.count(data, offsets.to(torch.int32))
    with pytest.raises(RuntimeError, match="at least one"):
        adv.count(data, offsets[:0])
    with pytest.raises(RuntimeError, match="UTF-8"):
        adv(["oil", "a \ud800 b"])
