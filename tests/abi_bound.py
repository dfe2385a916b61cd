"""The check that the per-family ABI test files share: an entry point is declared in include/gcnk.h with the
argument count the test states, is in _lib.SIGNATURES with as many, and the loaded library's function carries those
argtypes and that restype.  The counts are typed in the test files by hand: they, the `== 13` and the struct byte
layouts of test_keep_abi.py / test_epoch_abi.py / test_train_ref.py pin what _lib reads from the header against
numbers counted independently of it.  No GPU."""
import os
import re

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    """include/gcnk.h -> (its text, the text without comments)."""
    with open(os.path.join(ROOT, "include", "gcnk.h")) as f:
        text = f.read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def assert_declared_exported_bound(names, restype=None, newer=True):
    """names: entry point -> its argument count, the stream included.  ``restype``: the ctypes class each must
    return, where the test states one.  ``newer``: each was added within ABI 13, so a variant library may lack it."""
    src = header()[1]
    lib = _lib.load()
    for name, nargs in names.items():
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert decl and (nargs == 0 or len(decl.group(1).split(",")) == nargs), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert (name in _lib.NEWER_THAN_SOME_VARIANTS) == newer, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0]
        assert restype is None or fn.restype is restype
    assert lib.gcnk_abi_version() == _lib.ABI_VERSION == 13
