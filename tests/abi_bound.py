"""The check that the per-family ABI test files share: an entry point is declared in the public header the test names
(include/gcnk.h, or the family header it includes) with the argument count the test states, is in _lib.SIGNATURES
with as many, and the loaded library's function carries those argtypes and that restype.  The counts are typed in the
test files by hand: they, the `== 13` and the struct byte layouts of test_keep_abi.py / test_epoch_abi.py /
test_train_ref.py pin what _lib reads from the headers against numbers counted independently of it.  No GPU."""
import os
import re

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name=None):
    """What a C caller of include/gcnk.h sees, every public header in include order -- or the one header ``name``
    (a basename) -> (its text, the text without comments)."""
    texts = []
    for path in _lib.HEADERS:
        if name in (None, os.path.basename(path)):
            with open(path) as f:
                texts.append(f.read())
    assert texts, name
    text = "".join(texts)
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


_header = header   # (assert_declared_exported_bound's ``header`` argument hides the function)


def declared_names(name):
    """Every gcnk_* function that the header ``name`` declares, by a regex of the test's own."""
    return set(re.findall(r"\b(gcnk_[a-z0-9_]+)\s*\(", header(name)[1]))


def assert_declared_exported_bound(names, restype=None, newer=True, header="gcnk.h"):
    """names: entry point -> its argument count, the stream included.  ``restype``: the ctypes class each must
    return, where the test states one.  ``newer``: each was added within ABI 13, so a variant library may lack it.
    ``header``: the basename of the public header that declares them."""
    src = _header(header)[1]
    lib = _lib.load()
    for name, nargs in names.items():
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert decl and (nargs == 0 or len(decl.group(1).split(",")) == nargs), name
        assert _lib.DECLARED_IN[name] == header
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert (name in _lib.NEWER_THAN_SOME_VARIANTS) == newer, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0]
        assert restype is None or fn.restype is restype
    assert lib.gcnk_abi_version() == _lib.ABI_VERSION == 13
