"""What the Python package binds of include/gcnk.h and the family headers it includes, as sorted text: diff the
output of two trees to see what a change did to the ABI (profiles/r34_abi_dump_*.txt: the tree that typed the tables
by hand against the tree that reads the header; profiles/r43_abi_headers_dump_*.txt: three tables and headers
against one table and a header per family -- no difference either time).  No GPU and no library needed: nothing is
loaded.  It runs on an older tree too: copy it there (a tree from before _lib.HEADERS kept the family headers'
entry points in tables of their own, and named no header but gcnk.h).

  python scripts/abi_dump.py
      func <name> <restype> <argtypes ...>          every entry point the package binds, ctypes class names
      struct <name> <size>                          every ctypes.Structure that _lib or record holds, under its
      field <struct> <field> <offset> <size> <type>   Python name (and a derived struct without one under its C name)
      const <NAME> <value>                          every object-like `#define GCNK_<NAME>` of the headers with the
                                                    value the package (_lib, else ops, else record) gives <NAME>,
                                                    or `unbound`
"""
import ctypes
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lines():
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import _lib, ops, record
    # (_lib.SIGNATURES, and on a tree from before _lib.HEADERS the family headers' tables beside it)
    tables = [table for attr, table in vars(_lib).items() if attr.endswith("SIGNATURES")]
    bound = {name: signature for table in tables for name, signature in table.items()}
    out = [" ".join(["func", name, res.__name__] + [a.__name__ for a in args]) for name, (res, args) in bound.items()]
    structs = {attr: cls for mod in (_lib, record) for attr, cls in vars(mod).items()
               if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure}
    structs.update({c: cls for c, cls in getattr(_lib, "STRUCTS", {}).items() if cls not in structs.values()})
    shown = {cls: name for name, cls in structs.items()}   # (a nested struct under the name it is listed by)
    for name, cls in structs.items():
        out.append(f"struct {name} {ctypes.sizeof(cls)}")
        for field, ctype in cls._fields_:
            at = getattr(cls, field)
            out.append(f"field {name} {field} {at.offset} {at.size} {shown.get(ctype, ctype.__name__)}")
    names = []
    for path in getattr(_lib, "HEADERS", None) or sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        with open(path) as f:
            names += re.findall(r"^#define GCNK_(\w+)[ \t]+\S", f.read(), flags=re.M)
    for name in names:
        value = next((getattr(m, name) for m in (_lib, ops, record) if hasattr(m, name)), "unbound")
        out.append(f"const {name} {value}")
    return sorted(out)


if __name__ == "__main__":
    print("\n".join(lines()))
