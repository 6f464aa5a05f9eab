"""CPU test of the C ABI's surface: every function include/g2s.h and include/g2s_test.h declare resolves in the loaded
library.  The ABI is implemented by several units of gap2seq_amd/csrc (g2s_api.hip and the api_*.hip files); an entry
point or a test hook that is in none of them fails here by name."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return set(re.findall(r"\b(g2s_[a-z0-9_]+)\s*\(", text))


def test_every_declared_function_resolves(product):
    so = ctypes.CDLL(product.library_path())
    names = declared_functions("g2s.h") | declared_functions("g2s_test.h")
    assert names == set(product._SIGS)  # (nothing the regex missed: the ctypes binding lists the same functions)
    missing = []
    for n in sorted(names):
        try:
            getattr(so, n)
        except AttributeError:
            missing.append(n)
    assert not missing, "declared in include/*.h, not in libg2s_hip.so: %s" % ", ".join(missing)
