"""The one ctypes binding layer of the eight shared libraries: every signature is read from the C header that declares it.

The compiler ties header and implementation (each .hip unit includes its header); `prototypes` ties the binding to the same text, so no entry point is described
by hand a second time.  The type rule, applied to a parameter after dropping `const` and its name:
  no `*`   int / int32_t -> c_int, int64_t -> c_int64, size_t -> c_size_t, float, double, unsigned / uint32_t -> c_uint, uint64_t -> c_uint64
  one `*`  a struct the caller registered -> POINTER(cls);  `const char*` as a RETURN type -> c_char_p;  anything else -> c_void_p
           (device pointers, the opaque nl_frame*, and host out-pointers: ctypes takes byref(...) and arrays for a c_void_p parameter)
  two `*`  POINTER(c_void_p)
Whatever else it meets raises and names the header and the prototype; nothing defaults to void*.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import torch  # noqa: F401  -- MUST precede CDLL: torch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1 (same
# SONAMEs as /opt/rocm's); loading ours first would put two HIP runtimes in the process and every torch pointer
# would be foreign to our kernels.  Importing torch first makes the dynamic loader resolve our DT_NEEDED to its copy.

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")   # a header given by file name is looked up here

_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
            "unsigned": C.c_uint, "uint32_t": C.c_uint, "uint64_t": C.c_uint64}


@functools.lru_cache(maxsize=None)
def _code(header):
    """The header's text without comments (each becomes one space, so a `#define` keeps its line); read once per process."""
    with open(os.path.join(INCLUDE, header)) as f:
        return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def _ctype(base, stars, structs, where, ret=False):
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1:
        return C.POINTER(structs[base]) if base in structs else C.c_char_p if ret and base == "char" else C.c_void_p
    if stars == 2:
        return C.POINTER(C.c_void_p)
    raise TypeError(f"{where}: no ctypes rule for `{base}{'*' * stars}`")


def _declarator(text, structs, where, ret=False):
    """`const float* const* tensors` -> POINTER(c_void_p): one type, at most one name, no array."""
    words = [w for w in re.findall(r"\w+", text) if w != "const"]
    if re.search(r"[^\w\s*]", text) or not 1 <= len(words) <= (1 if ret else 2):
        raise TypeError(f"{where}: cannot read `{text.strip()}`")
    return _ctype(words[0], text.count("*"), structs, where, ret)


def prototypes(header, prefix, structs=None):
    """[(name, restype, argtypes)] of every `ret name(args);` of the header whose name starts with `prefix`, in header order."""
    structs, out = structs or {}, []
    code = re.sub(r"^[ \t]*#[^\n]*", " ", _code(header), flags=re.M)
    for m in re.finditer(r"([A-Za-z_][\w\s*]*?)\b(%s\w*)\s*\(([^()]*)\)\s*;" % re.escape(prefix), code):
        ret, name, args = m.groups()
        where = f"{os.path.basename(header)}: {' '.join(m.group(0).split())}"
        args = [] if args.strip() == "void" else [_declarator(a, structs, where) for a in args.split(",")]
        out.append((name, _declarator(ret, structs, where, ret=True), args))
    return out


def defines(header):
    """{NAME: int | float} of every `#define NAME <integer>[u]` and `#define NAME <float>f`."""
    out = {}
    for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S+)[ \t]*$", _code(header), flags=re.M):
        if re.fullmatch(r"\d+[uU]?", val):
            out[name] = int(val.rstrip("uU"))
        elif re.fullmatch(r"\d+\.\d*(e[-+]?\d+)?f", val):
            out[name] = float(val[:-1])
    return out


def struct_fields(header, structs=None):
    """{struct_name: [(field, ctype)]} of every `typedef struct { ... } name;`, by the type rule above; `int32_t reserved[4]` -> c_int32 * 4."""
    structs, out = structs or {}, {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", _code(header)):
        fields = out[name] = []
        for stmt in filter(str.strip, body.split(";")):
            where = f"{os.path.basename(header)}: {name}: {' '.join(stmt.split())}"
            m = re.fullmatch(r"\s*((?:const\s+)?\w+)(.*)", stmt, flags=re.S)   # the base type, then the declarators: `V, H, Wimg` / `* const* weights` / `reserved[4]`
            for decl in m.group(2).split(","):
                d = re.fullmatch(r"([\s*]|const\b)*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", decl)
                if not d:
                    raise TypeError(f"{where}: cannot read `{decl.strip()}`")
                t = _ctype(m.group(1).split()[-1], decl.count("*"), structs, where)
                fields.append((d.group(2), t * int(d.group(3)) if d.group(3) else t))
    return out


def bind(lib_path, header, prefix, abi_fn, abi_define, binding_abi, structs=None, what="there is no CPU fallback"):
    """CDLL(lib_path) with restype / argtypes of every prototype of the header set; raises if the file or an export is missing, or unless the library's
    abi_fn(), the header's abi_define and the binding's own written number are one number."""
    if not os.path.exists(lib_path):
        raise RuntimeError(f"{lib_path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` ({what})")
    lib = C.CDLL(lib_path)
    for name, res, args in prototypes(header, prefix, structs):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got, want = getattr(lib, abi_fn)(), defines(header).get(abi_define)
    if not got == want == binding_abi:
        raise RuntimeError(f"{os.path.basename(lib_path)} ABI version mismatch: header {want}, library {got}, binding {binding_abi}")
    return lib


def stream(dev) -> int:
    """The hipStream_t of torch's current stream on `dev`, as the libraries' `void* stream`."""
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(t):
    """A tensor's device address for an optional pointer argument: None (NULL) for None."""
    return None if t is None else t.data_ptr()


def workspace(nbytes: int, device, what: str, error=RuntimeError) -> torch.Tensor:
    """The byte tensor for a `*_workspace_bytes` answer; 0 is the library's refusal of the shape or option: error(what)."""
    if nbytes == 0:
        raise error(what)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def dense_f32(t, what):
    """t, if it is what the libraries read through a `const float*`: fp32, contiguous, on a HIP device; ValueError otherwise."""
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous fp32 tensor on a HIP device")
    return t
