"""ctypes binding of libpcc_hip.so (the C-ABI declared in include/pcc_hip.h).

The library is built in-tree by ``build()`` (``make -C csrc``; hipcc --offload-arch=gfx950) and
must be present for any operator call: there is no CPU fallback and no second backend.  A
missing or unloadable library raises ``RuntimeError`` at first use.
"""
import ctypes
import os
import re
import types

from ._build import SO_PATH, build, check_kernel_resources, check_small_kernel_lds_reads, lint_lds_reads  # noqa: F401

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "pcc_hip.h")
_lib = None

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def parse_header(text):
    """The C ABI of a header as ctypes reads it: -> ({function: (restype, [(parameter name, type), ...])}, {constant: int}) for
    every ``pcc_*`` prototype and every integer ``#define PCC_*`` (the PCC_ prefix dropped).  int, int32_t, int64_t and float map
    to their ctypes twins, ``char*`` to c_char_p, every other pointer to c_void_p.  Anything else raises ValueError: a type this
    does not know or a statement it cannot read is never guessed at."""
    def ctype(t):
        t = re.sub(r"\s+", " ", re.sub(r"\s*\*\s*", "*", t)).strip()
        t = t[6:] if t.startswith("const ") else t
        if t in _SCALARS:
            return _SCALARS[t]
        if re.fullmatch(r"\w+\*", t):
            return ctypes.c_char_p if t == "char*" else ctypes.c_void_p
        raise ValueError(f"pcc_hip.h: unknown type `{t}`")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    defines = re.finditer(r"^[ \t]*#[ \t]*define[ \t]+PCC_(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)
    consts = {m.group(1): int(m.group(2)) for m in defines}
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text).replace("}", "")
    protos = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(pcc_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise ValueError(f"pcc_hip.h: cannot read `{stmt}`")
        params = []
        for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            pm = re.fullmatch(r"(.*[\s*])(\w+)", p.strip(), flags=re.S)
            if not pm:
                raise ValueError(f"pcc_hip.h: cannot read parameter `{p.strip()}` of {m.group(2)}")
            params.append((pm.group(2), ctype(pm.group(1))))
        protos[m.group(2)] = (ctype(m.group(1)), params)
    return protos, consts


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes binding is read from the C header, which ships beside the package")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


PROTOTYPES, _constants = _read_header()
# name -> (restype, argtypes), as include/pcc_hip.h declares them
SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in PROTOTYPES.items()}
# the header's integer constants without their prefix: PCC.OK, PCC.ERR_*, PCC.ACT_*, PCC.COORD_LIMIT, PCC.BATCH_LIMIT, PCC.COUNT_ERR_RANGE
PCC = types.SimpleNamespace(**_constants)


def lib():
    """The loaded library, an object with one callable per declared function; raises if it has not been built.  Every function
    is bound as a prototype with parameter flags, so ctypes checks the argument count before the call (a plainly bound cdecl
    function accepts surplus arguments, and a caller that kept the longer form of a prototype that had shrunk crashed the
    process): a surplus or missing argument raises TypeError.  ctypes skips the check for the prototypes without parameters; a
    surplus argument to those cannot corrupt anything.  The calls release the interpreter lock like CDLL's own."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the codec operators.")
        dll = ctypes.CDLL(SO_PATH)
        L = types.SimpleNamespace(_dll=dll)
        for name, (res, params) in PROTOTYPES.items():
            proto = ctypes.CFUNCTYPE(res, *(t for _, t in params))
            setattr(L, name, proto((name, dll), tuple((1, pname) for pname, _ in params)))   # AttributeError if not exported
        _lib = L
    return _lib


class PccError(RuntimeError):
    pass


def check(rc):
    if rc < 0:
        raise PccError(f"libpcc_hip: error {rc}: {lib().pcc_last_error().decode(errors='replace')}")
    return rc


def ptr(t):
    """Device (or host) pointer of a tensor / numpy array, or NULL."""
    if t is None:
        return None
    try:
        return t.data_ptr()
    except AttributeError:
        return t.ctypes.data


_raw_stream = None


def stream():
    """Raw handle of the calling thread's current HIP stream on the current device.  Asked for at every launch (~230 times
    per frame): torch.cuda.current_stream() builds a Stream object through several Python layers (8.6 us, 2 ms per
    frame); the two C calls below return the same handle in well under a microsecond."""
    global _raw_stream
    if _raw_stream is None:
        import torch
        try:
            get_stream, get_dev = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice
            get_stream(get_dev())
            _raw_stream = lambda: get_stream(get_dev())
        except AttributeError:                      # a torch build without the private accessors
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream
    return _raw_stream()
