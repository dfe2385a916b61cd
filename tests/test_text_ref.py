"""tests/text_ref.py, the restatement the word counter's GPU tests take their expected arrays from, pinned without
a GPU: to sklearn's recorded transform (tests/golden/text_r8_small.npz), to CountVectorizer.transform itself where
sklearn is installed (the fixture and the adversarial texts), its white-space sets to Python's own ``re``; and the
host half of the package against it: the vocabulary table gcnk_text_table_build writes against the restatement's
table, byte for byte, and ``pack_host`` against ``encode``."""
import re

import numpy as np
import pytest

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib, text_count

import text_ref as R


@pytest.fixture(scope="module")
def gold():
    return R.golden()


def _sklearn(words):
    fe = pytest.importorskip("sklearn.feature_extraction.text")
    return fe.CountVectorizer(vocabulary=words, token_pattern=r"\S+", lowercase=False)


def _equal(ours, X):
    X = X.tocsr()
    X.sort_indices()
    assert ours[0].dtype == np.int32 and ours[1].dtype == np.int32 and ours[2].dtype == np.float64
    assert np.array_equal(ours[0], X.indptr) and np.array_equal(ours[1], X.indices) and np.array_equal(ours[2], X.data)


def test_white_space_sets_are_pythons():
    spaces = [cp for cp in range(0x110000) if re.fullmatch(r"\s", chr(cp))]
    assert len(spaces) == 29
    assert tuple(cp for cp in spaces if cp < 0x80) == R.ASCII_SPACE
    assert tuple(cp for cp in spaces if cp >= 0x80) == R.NON_ASCII_SPACE == text_count.NON_ASCII_SPACE
    assert len(R.ASCII_SPACE) == 10 and len(R.NON_ASCII_SPACE) == 19


def test_restatement_gives_the_recorded_transform(gold):
    assert len(gold["texts"]) == 300 and len(gold["words"]) == len(set(gold["words"])) == int(gold["vocab_offsets"].size - 1)
    ours = R.count(gold["text_bytes"].tobytes(), gold["text_offsets"], R.vocabulary_of(gold["words"]))
    assert np.array_equal(ours[0], gold["indptr"]) and np.array_equal(ours[1], gold["indices"])
    assert np.array_equal(ours[2], gold["data"].astype(np.float64)) and gold["data"].dtype == np.int64
    # the fixture is what the issue asks for: rows ascending, unseen words in the last 100 documents
    for d in range(300):
        row = gold["indices"][gold["indptr"][d]:gold["indptr"][d + 1]]
        assert (np.diff(row) > 0).all()
    vocab = R.vocabulary_of(gold["words"])
    data, off = gold["text_bytes"].tobytes(), gold["text_offsets"]
    assert any(t not in vocab for d in range(200, 300) for t in R.tokens(data[off[d]:off[d + 1]]))
    assert R.encode(gold["texts"])[0] == data and np.array_equal(R.encode(gold["texts"])[1], off)


def test_restatement_against_sklearn_on_the_fixture(gold):
    _equal(R.transform(gold["texts"], gold["words"]), _sklearn(gold["words"]).transform(gold["texts"]))


def test_restatement_against_sklearn_on_the_adversarial_texts():
    ours = R.transform(R.ADVERSARIAL_TEXTS, R.ADVERSARIAL_WORDS)
    _equal(ours, _sklearn(R.ADVERSARIAL_WORDS).transform(R.ADVERSARIAL_TEXTS))
    assert ours[0][-1] > 60          # (the list does count something)
    # piece boundaries and documents packed without a separator, as the GPU tests build them
    texts = ["x" * i + " oil " + "y" * i + "price" for i in range(131)] + ["crude oil", "price oil"]
    _equal(R.transform(texts, R.ADVERSARIAL_WORDS), _sklearn(R.ADVERSARIAL_WORDS).transform(texts))


def test_restatement_by_hand():
    words = ["oil", "price", "caf\u00e9"]
    ip, ix, ct = R.transform(["price oil  price\toil\x1coil", "", "Oil oils caf\u00e9\u3000caf\u00e9 pric", "oil"], words)
    assert ip.tolist() == [0, 2, 2, 3, 4] and ix.tolist() == [0, 1, 2, 0] and ct.tolist() == [3.0, 2.0, 2.0, 1.0]
    # documents are delimited by offsets: "oil" + "price" side by side do not merge
    ip, ix, ct = R.count(b"crude oilprice oil", np.array([0, 9, 18]), R.vocabulary_of(["oil", "price", "oilprice"]))
    assert ip.tolist() == [0, 1, 3] and ix.tolist() == [0, 0, 1] and ct.tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(UnicodeEncodeError):
        R.encode(["a \ud800 b"])


def test_hash_and_collision_search():
    assert R.fnv1a(b"") == 0x811C9DC5 and R.fnv1a(b"a") == 0xE40C292C and R.fnv1a(b"foobar") == 0xBF9CF968
    a, b = R.colliding_pair()
    assert a != b and len(a) == len(b) == 6 and R.fnv1a(a.encode()) == R.fnv1a(b.encode())
    tab = R.table([a.encode(), b"oil", b.encode()])
    assert R.lookup(tab, a.encode()) == 0 and R.lookup(tab, b.encode()) == 2 and R.lookup(tab, b"oil") == 1
    only_a = R.table([a.encode(), b"oil"])
    assert R.lookup(only_a, a.encode()) == 0 and R.lookup(only_a, b.encode()) is None   # the hash alone is no match


@pytest.mark.parametrize("which", ["fixture", "adversarial", "colliding", "one"])
def test_host_table_builder_against_the_restatement(gold, which):
    a, b = R.colliding_pair()
    words = {"fixture": gold["words"], "adversarial": R.ADVERSARIAL_WORDS, "colliding": [b, "oil", a, "price"],
             "one": ["x"]}[which]
    tab, V, slots, longest, blob_bytes = text_count.build_table(words)
    want = R.table([w.encode("utf-8") for w in words])
    assert tab.dtype == np.uint8 and np.array_equal(tab, want)
    enc = [w.encode("utf-8") for w in words]
    assert (V, slots, longest, blob_bytes) == (len(words), R.slots_for(len(words)), max(map(len, enc)), sum(map(len, enc)))
    lib = _lib.load()
    assert lib.gcnk_text_table_slots(V) == slots and lib.gcnk_text_table_bytes(blob_bytes, V) == tab.size
    for i, w in enumerate(enc):
        assert R.lookup(tab, w) == i and R.lookup(tab, w + b"s") in (None, *[j for j, x in enumerate(enc) if x == w + b"s"])


def test_host_table_builder_refusals():
    for words, what in (([], "at least one word"), (["oil", ""], "empty"), (["oil", "price", "oil"], "the same")):
        with pytest.raises(RuntimeError, match=what):
            text_count.build_table(words)
    a, b = R.colliding_pair()
    with pytest.raises(RuntimeError, match="the same"):
        text_count.build_table([a, b, a])
    text_count.build_table([a, b])          # equal hashes are no duplicate
    with pytest.raises(RuntimeError, match="UTF-8"):
        text_count.build_table(["oil", "\ud800"])
    with pytest.raises(RuntimeError, match="str"):
        text_count.build_table(["oil", b"price"])


def test_vocabulary_words():
    assert text_count.vocabulary_words({"b": 1, "a": 0, "c": np.int64(2)}) == ["a", "b", "c"]
    assert text_count.vocabulary_words(("x", "y")) == ["x", "y"]
    for bad in ({"a": 0, "b": 2}, {"a": 1, "b": 1}, {"a": -1, "b": 0}, {"a": 0.5, "b": 0}, "oil"):
        with pytest.raises(RuntimeError, match="vocabulary"):
            text_count.vocabulary_words(bad)


def test_pack_host_against_encode(gold):
    for texts in (gold["texts"], R.ADVERSARIAL_TEXTS, [], [""], ["", "", ""], ["", "a", "", "b c", ""]):
        data, off = text_count.pack_host(texts)
        want, want_off = R.encode(texts)
        assert data.dtype == np.uint8 and off.dtype == np.int64
        assert data.tobytes() == want and np.array_equal(off, want_off)
    with pytest.raises(RuntimeError, match="UTF-8"):
        text_count.pack_host(["fine", "a \ud800 b"])
    with pytest.raises(RuntimeError, match="str"):
        text_count.pack_host(["fine", b"bytes"])
    with pytest.raises(RuntimeError, match="sequence"):
        text_count.pack_host("one string")
