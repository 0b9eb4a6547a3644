"""CPU-side tests of the binding layer (nerf_loc_amd/_cabi.py): the parser on a header written here, every prototype, struct and #define of the three real
headers, four signatures typed out by hand as the independent witness, and the refusals of bind()."""
import ctypes as C
import os
import re

import pytest

from nerf_loc_amd import _app_lib, _cabi, _head_lib, _lib

P, PP, I, L, Z, F, D, U, U64 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_size_t, C.c_float, C.c_double, C.c_uint, C.c_uint64
HEADERS = (("nerfloc_render.h", "nl_", 104, _lib), ("nerfloc_head.h", "nlh_", 7, _head_lib), ("nerfloc_app.h", "nla_", 8, _app_lib))

SYNTHETIC = """\
/* a header: int t_in_a_comment(int x); */
#ifndef T_H
#define T_H
#include <stdint.h>
#define T_ABI_VERSION 3u   /* a trailing comment, over
                            * two lines */
#define T_LIMIT 50.0f
#define T_COUNT 6
#define T_ALIAS t_other    // not a number
#ifdef __cplusplus
extern "C" {
#endif
typedef struct t_cfg { int32_t W, C; float eps; const float* rows; float* const* grads;   /* HOST */
  int32_t reserved[4]; const void* more[1]; } t_cfg;
typedef struct t_frame t_frame;   /* opaque */
typedef struct t_job {
  const t_cfg* cfg;
  const t_frame* frame;
  int64_t R; size_t bytes; uint32_t flags;
} t_job;
int t_version(void);
const char* t_strerror(int status);
// int t_in_a_line_comment(int x);
size_t t_bytes(const t_cfg* cfg, int64_t N,
               int32_t V /* views, at most 16 */, unsigned flags,
               uint32_t more, uint64_t seed);   // the sizes
int t_run(const t_cfg* cfg, const float* const* tensors, t_frame** out, const t_frame* frame, float eps, double thr, int* host_count /* HOST */,
          void* stream);
int other_fn(int a);
#ifdef __cplusplus
}
#endif
#endif
"""


class Cfg(C.Structure):
    pass


@pytest.fixture()
def header(tmp_path):
    def write(text, name="t.h"):
        path = tmp_path / name
        path.write_text(text)
        return str(path)
    return write


def test_parser_applies_every_rule_to_a_written_header(header):
    h = header(SYNTHETIC)
    cfg = C.POINTER(Cfg)
    assert _cabi.prototypes(h, "t_", {"t_cfg": Cfg}) == [
        ("t_version", I, []),                                   # (void)
        ("t_strerror", C.c_char_p, [I]),                        # const char* as a return type
        ("t_bytes", Z, [cfg, L, I, U, U, U64]),                 # several lines, a comment with a comma between arguments
        ("t_run", I, [cfg, PP, PP, P, F, D, P, P]),             # a registered struct, two stars twice, the opaque frame, a host out-pointer
    ]                                                           # and nothing of other_fn or of the two commented prototypes
    assert [n for n, _, _ in _cabi.prototypes(h, "other_")] == ["other_fn"]
    assert _cabi.prototypes(h, "t_")[2][2][0] is P              # an unregistered struct pointer is a void pointer


@pytest.mark.parametrize("proto", ["int t_bad(long n);", "int t_bad(nl_config cfg);", "int t_bad(float x[3]);", "int t_bad(float*** x);",
                                   "int t_bad(unsigned int n);", "void t_bad(int n);", "char t_bad(int n);"])
def test_parser_refuses_what_the_rule_does_not_know(header, proto):
    with pytest.raises(TypeError, match=r"t\.h: .*t_bad"):
        _cabi.prototypes(header("int t_good(int n);\n" + proto + "\n"), "t_")


def test_defines_have_the_python_type_of_the_literal(header):
    d = _cabi.defines(header(SYNTHETIC))
    assert d == {"T_ABI_VERSION": 3, "T_LIMIT": 50.0, "T_COUNT": 6}
    assert type(d["T_ABI_VERSION"]) is int and type(d["T_COUNT"]) is int and type(d["T_LIMIT"]) is float
    r = _cabi.defines("nerfloc_render.h")
    assert type(r["NL_RENDER_FLAGS_ALL"]) is int and r["NL_RENDER_FLAGS_ALL"] == 3 and type(r["NL_GUARD_LOGIT_LIMIT_F16MX"]) is float
    assert r["NL_ABI_VERSION"] == _lib.ABI_VERSION and _cabi.defines("nerfloc_app.h")["NLA_FILM_CLIP01"] == 1


def test_struct_fields_of_a_written_header(header):
    s = _cabi.struct_fields(header(SYNTHETIC), {"t_cfg": Cfg})
    assert list(s) == ["t_cfg", "t_job"]
    assert s["t_cfg"] == [("W", C.c_int32), ("C", C.c_int32), ("eps", F), ("rows", P), ("grads", PP), ("reserved", C.c_int32 * 4), ("more", P * 1)]
    assert s["t_job"] == [("cfg", C.POINTER(Cfg)), ("frame", P), ("R", L), ("bytes", Z), ("flags", C.c_uint32)]
    with pytest.raises(TypeError, match="t_s"):
        _cabi.struct_fields(header("typedef struct t_s { long n; } t_s;", "u.h"))


@pytest.mark.parametrize("name, prefix, count, mod", HEADERS)
def test_every_prototype_of_the_real_headers_parses(name, prefix, count, mod):
    protos = _cabi.prototypes(name, prefix, getattr(mod, "STRUCTS", None))
    assert len(protos) == count and protos == mod.SYMBOLS
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(_cabi.INCLUDE, name)).read(), flags=re.S)   # the regex of the libraries' own boundary tests
    assert sorted(n for n, _, _ in protos) == sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, src)))
    assert all(res in (I, Z, L, C.c_char_p) for _, res, _ in protos)


def test_four_signatures_typed_out_by_hand():
    cfg, out, opts = C.POINTER(_lib.NlConfig), C.POINTER(_lib.NlRenderOut), C.POINTER(_lib.NlRenderOpts)
    render, head, app = (dict((n, (r, a)) for n, r, a in m.SYMBOLS) for m in (_lib, _head_lib, _app_lib))
    assert render["nl_render_rays_ex"] == (I, [cfg, P, P, P, P, P, P, L, I, out, P, Z, P, opts])
    assert render["nl_sct_backward_dropout"] == (I, [P, P, I, I, I, I, P, P, L, P, P, L, L, P, Z, P, P, P, P, P, P, PP, I, P, Z, F, U64, P])
    assert len(render["nl_sct_backward_dropout"][1]) == 28
    assert app["nla_film"] == (I, [P, P, L, L, I, U, P, P])
    assert head["nlh_pnp_ransac_counted"] == (I, [P, P, P, P, P, P, L, I, U64, I, P, P, P, P, P, Z, P])


def _shape(t):
    """(element type, array length or None) of a field's ctypes type."""
    return (t._type_, t._length_) if issubclass(t, C.Array) else (t, None)


def test_structure_classes_equal_the_headers_structs():
    parsed = _cabi.struct_fields("nerfloc_render.h", _lib.STRUCTS)
    assert set(parsed) == set(_lib.STRUCTS) and len(parsed) == 8          # every struct with a body has its class
    assert not _cabi.struct_fields("nerfloc_head.h") and not _cabi.struct_fields("nerfloc_app.h")
    for name, cls in _lib.STRUCTS.items():
        assert [(f, _shape(t)) for f, t in cls._fields_] == [(f, _shape(t)) for f, t in parsed[name]], name


def test_bind_refuses_a_wrong_number_a_missing_export_and_a_missing_file(header):
    args = ("nlh_", "nlh_abi_version", "NLH_ABI_VERSION")
    assert _cabi.bind(_head_lib.LIB_PATH, "nerfloc_head.h", *args, 1).nlh_abi_version() == 1
    with pytest.raises(RuntimeError, match="ABI version mismatch: header 1, library 1, binding 2"):       # the binding's written number is wrong
        _cabi.bind(_head_lib.LIB_PATH, "nerfloc_head.h", *args, 2)
    text = open(os.path.join(_cabi.INCLUDE, "nerfloc_head.h")).read()
    stale = header(text.replace("#define NLH_ABI_VERSION 1", "#define NLH_ABI_VERSION 2"))
    for binding in (1, 2):                                                                                # the header's define and the library disagree
        with pytest.raises(RuntimeError, match=f"ABI version mismatch: header 2, library 1, binding {binding}"):
            _cabi.bind(_head_lib.LIB_PATH, stale, *args, binding)
    with pytest.raises(RuntimeError, match="ABI version mismatch: header None"):
        _cabi.bind(_head_lib.LIB_PATH, header("int nlh_abi_version(void);", "nodefine.h"), *args, 1)
    with pytest.raises(AttributeError, match="nlh_not_there"):
        _cabi.bind(_head_lib.LIB_PATH, header(text.replace("int nlh_abi_version(void);", "int nlh_abi_version(void); int nlh_not_there(void);"), "more.h"), *args, 1)
    with pytest.raises(RuntimeError, match=r"nowhere\.so not found.*no CPU fallback"):
        _cabi.bind("/nowhere.so", "nerfloc_head.h", *args, 1)
