"""What the Python package binds of include/gcnk.h, as sorted text: diff the output of two trees to see what a
change did to the ABI (profiles/r34_abi_dump_*.txt: the tree that typed the tables by hand against the tree that
reads the header -- no difference).  No GPU and no library needed: nothing is loaded.

  python scripts/abi_dump.py
      func <name> <restype> <argtypes ...>          every entry of _lib.SIGNATURES, ctypes class names
      struct <name> <size>                          every ctypes.Structure that _lib or record holds, under its
      field <struct> <field> <offset> <size> <type>   Python name (and a derived struct without one under its C name)
      const <NAME> <value>                          every object-like `#define GCNK_<NAME>` of the header with the
                                                    value the package (_lib, else ops, else record) gives <NAME>,
                                                    or `unbound`
"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lines():
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import _lib, ops, record
    out = [" ".join(["func", name, res.__name__] + [a.__name__ for a in args])
           for name, (res, args) in _lib.SIGNATURES.items()]
    structs = {attr: cls for mod in (_lib, record) for attr, cls in vars(mod).items()
               if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure}
    structs.update({c: cls for c, cls in getattr(_lib, "STRUCTS", {}).items() if cls not in structs.values()})
    shown = {cls: name for name, cls in structs.items()}   # (a nested struct under the name it is listed by)
    for name, cls in structs.items():
        out.append(f"struct {name} {ctypes.sizeof(cls)}")
        for field, ctype in cls._fields_:
            at = getattr(cls, field)
            out.append(f"field {name} {field} {at.offset} {at.size} {shown.get(ctype, ctype.__name__)}")
    with open(os.path.join(ROOT, "include", "gcnk.h")) as f:
        names = re.findall(r"^#define GCNK_(\w+)[ \t]+\S", f.read(), flags=re.M)
    for name in names:
        value = next((getattr(m, name) for m in (_lib, ops, record) if hasattr(m, name)), "unbound")
        out.append(f"const {name} {value}")
    return sorted(out)


if __name__ == "__main__":
    print("\n".join(lines()))
