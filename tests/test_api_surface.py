"""CPU: every public name the binding had before it was split by object (tests/golden/api_names.txt, the sorted names of
``dir(api)`` without a leading underscore) is still reachable as ``api.NAME``, and a class or function that lives in
another module of the package is the same object there."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_names.txt")


def test_every_public_name_of_api_is_still_there():
    from mt_renderer_amd import api
    names = open(GOLDEN).read().split()
    assert len(names) >= 100 and names == sorted(set(names)), "the golden was not read"
    missing = [n for n in names if not hasattr(api, n)]
    assert not missing, missing
    for n in names:
        obj = getattr(api, n)
        home = getattr(obj, "__module__", None)
        if isinstance(home, str) and home.startswith("mt_renderer_amd.") and getattr(obj, "__name__", None) == n:
            assert getattr(sys.modules[home], n) is obj, (n, home)
    assert isinstance(api.EXPORTED_SYMBOLS, list) and len(api.EXPORTED_SYMBOLS) == len(set(api.EXPORTED_SYMBOLS)) == 130
