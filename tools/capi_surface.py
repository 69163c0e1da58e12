"""The public surface of a capi.py, as text: every public module-level name, the signature of every public Api attribute (and of the
underscore ones tests call), every ctypes.Structure's fields, types and size.  Two versions of the binding have the same surface if the
two listings are equal:

    git show HEAD~1:psgradientsdf_amd/capi.py > psgradientsdf_amd/capi_parent.py      (beside capi.py: the library paths are relative to the file)
    diff <(python tools/capi_surface.py psgradientsdf_amd/capi_parent.py) <(python tools/capi_surface.py psgradientsdf_amd/capi.py)
"""
import ctypes
import importlib.util
import inspect
import sys

KEPT = ("__init__", "_fn", "_check", "_view", "_settings", "ctx")      # Api's underscore names that tests use


def surface(path):
    spec = importlib.util.spec_from_file_location("capi_under_test", path)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    names = sorted(k for k in vars(m) if not k.startswith("_"))
    yield "names: " + " ".join(names)
    for k in names:
        v = getattr(m, k)
        if inspect.isclass(v) and issubclass(v, ctypes.Structure):
            yield f"struct {k} {ctypes.sizeof(v)}: " + ", ".join(f"{f} {getattr(t, '__name__', t)}" for f, t in v._fields_)
        elif inspect.isfunction(v):
            yield f"def {k}{inspect.signature(v)}"
        elif not inspect.isclass(v) and not inspect.ismodule(v):
            yield f"{k} = {v!r}"
    for k in sorted(k for k in vars(m.Api) if not k.startswith("_") or k in KEPT):
        v = inspect.getattr_static(m.Api, k)
        yield f"Api.{k}{inspect.signature(v.__func__ if isinstance(v, staticmethod) else v) if callable(getattr(m.Api, k)) else ' = ' + repr(v)}"


if __name__ == "__main__":
    print("\n".join(surface(sys.argv[1])))
