"""Parser of the prototypes of include/mfhip.h, shared by the ABI tests (a plain helper module, like gemm_ref.py).

Kinds: 'p' pointer, 'i' int / int32_t, 'l' int64_t, 'f' float; a return may also be 's' (const char*) or 'v' (void).  A pointer to one of
the host descriptor structs (mf_*_desc, and mf_gemm_plan / mf_wgrad_plan / mf_gn_plan, which the library fills) is given as the struct's C name instead of 'p';
mf_sched_row and mf_program are not descriptors (the first lives in device memory, the second is opaque)."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfhip.h")

_SCALARS = {"int": "i", "int32_t": "i", "int64_t": "l", "float": "f"}


def _code(path: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", text, flags=re.M)


def declared_names(path: str = HEADER) -> list:
    """Every mf_* identifier that is followed by '(' in the header's code: what the prototypes below must cover."""
    return sorted(set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", _code(path))))


def _param_kind(decl: str) -> str:
    words = decl.replace("*", " * ").split()
    if "*" in words:
        desc = [w for w in words if re.fullmatch(r"mf_\w+_desc|mf_gemm_plan|mf_wgrad_plan|mf_gn_plan", w)]
        return desc[0] if desc else "p"
    scalar = [w for w in words if w != "const"]
    if not scalar or scalar[0] not in _SCALARS:
        raise ValueError(f"mfhip.h: parameter {decl!r} has a type the ABI tests know no kind for")
    return _SCALARS[scalar[0]]


def prototypes(path: str = HEADER) -> dict:
    """name -> (return kind, [one kind per parameter, the stream included]) for every function the header declares."""
    out = {}
    for m in re.finditer(r"([\w ]+?\**)\s*\b(mf_\w+)\s*\(([^(){};]*)\)\s*;", _code(path)):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        if ret == "const char*":
            rk = "s"
        elif ret == "void":
            rk = "v"
        elif ret in _SCALARS and ret != "float":
            rk = _SCALARS[ret]
        else:
            raise ValueError(f"mfhip.h: {name} returns {ret!r}, a type the ABI tests know no kind for")
        if name in out:
            raise ValueError(f"mfhip.h declares {name} twice")
        out[name] = (rk, [] if params in ("", "void") else [_param_kind(p) for p in params.split(",")])
    return out
