"""CPU tests of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports every symbol
include/ossid_hip.h declares (no compute calls -- there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ossid_hip.h")).read()


def _declared():
    text = _header()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ossid_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_entry_points():
    names = _declared()
    for must in ("ossid_zephyr_featurize", "ossid_zephyr_project_uv", "ossid_pn2_score", "ossid_zephyr_prep_frame_u8"):
        assert must in names


def test_library_exports_every_declared_symbol(hiplib):
    handle = ctypes.CDLL(os.path.join(ROOT, "ossid_code_amd", "libossid_hip.so"))
    missing = [n for n in _declared() if not hasattr(handle, n)]
    assert not missing, missing


def test_python_prototypes_cover_the_header(hiplib):
    assert set(_declared()) == set(hiplib.exported_symbols())


def _gcc(tmp_path, name, body, *flags):
    """Compiles body (behind the header's #include) as C; returns gcc's exit status and messages."""
    import subprocess
    src = tmp_path / name
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ossid_hip.h"\n' + body)
    out = subprocess.run(["gcc", "-std=c11", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)] + list(flags),
                         capture_output=True, text=True)
    return out.returncode, out.stderr


def _parsed():
    from ossid_code_amd import _abi
    return _abi.parse(_header())


def test_abi_version_and_struct_layouts_agree_between_header_and_binding(hiplib, tmp_path):
    """OSSID_ABI_VERSION of the header = the binding's = what the built library reports, and every descriptor struct has
    the same size, and EVERY field the same offset and size, when gcc compiles the header as in the ctypes class."""
    import subprocess
    text = _header()
    ver = int(re.search(r"#define\s+OSSID_ABI_VERSION\s+(\d+)", text).group(1))
    assert ver == hiplib.ABI_VERSION == hiplib.lib().ossid_abi_version(None, 0)
    structs = _parsed()[1]
    assert sorted(structs) == sorted(re.findall(r"typedef\s+struct\s+(\w+)", text)) == sorted(hiplib._STRUCT_NAMES)
    assert len(structs) >= 6 and "ossid_seq_op" in structs
    body = "".join('printf("%%zu\\n", sizeof(%s));\n' % c +
                   "".join('printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));\n' % (c, f, c, f) for f, _, _ in fields)
                   for c, fields in structs.items())
    exe = tmp_path / "layout"
    rc, err = _gcc(tmp_path, "layout.c", "int main(void) {\n%sreturn 0;\n}\n" % body, "-o", str(exe))
    assert rc == 0, err
    lines = iter(subprocess.check_output([str(exe)]).decode().split("\n"))
    for c, fields in structs.items():
        st = getattr(hiplib, hiplib._STRUCT_NAMES[c])
        assert [n for n, _ in st._fields_] == [f for f, _, _ in fields]
        assert int(next(lines)) == ctypes.sizeof(st), c
        for f, _, _ in fields:
            off, size = (int(v) for v in next(lines).split())
            assert (off, size) == (getattr(st, f).offset, getattr(st, f).size), (c, f, off, size)


def _prototype_checks(protos):
    return "".join("{ %s (*p)(%s) = %s; (void)p; }\n" % (ret, ", ".join(params) or "void", name)
                   for name, (ret, params) in protos.items())


def test_every_prototype_type_and_constant_is_what_gcc_reads_in_the_header(hiplib, tmp_path):
    """gcc is the judge of what the reader made of the header: each of the entry points is assigned to a function pointer
    spelled with the reader's return and parameter types (a dropped, merged, reordered or mistyped parameter does not
    compile), each scalar of the type table has the size, signedness and float / integer class of its ctypes type, and each OSSID_*
    constant its value. The binding hands exactly these types and values on."""
    from ossid_code_amd import _abi
    consts, _, protos = _parsed()
    assert len(protos) >= 153 and set(protos) == set(_declared())
    floats = {"float": ctypes.c_float, "double": ctypes.c_double}
    checks = _prototype_checks(protos)
    for t, ct in _abi.SCALARS.items():
        # Seq._compile: float and double travel as floating-point arguments, every other scalar in a 64-bit integer slot
        assert (ct is floats[t]) if t in floats else (ct not in floats.values() and ctypes.sizeof(ct) <= 8), t
        checks += '_Static_assert(sizeof(%s) == %d, "%s");\n' % (t, ctypes.sizeof(ct), t)
        checks += '_Static_assert(((%s)0.5 != 0) == %d && ((%s)-1 < 0) == %d, "%s");\n' % (t, t in floats, t, ct(-1).value < 0, t)
    assert hiplib._f is ctypes.c_float and _abi.ctype("double") is ctypes.c_double
    checks += '_Static_assert(sizeof(void*) == %d && sizeof(char*) == %d, "pointers");\n' % (
        ctypes.sizeof(_abi.ctype("const float*")), ctypes.sizeof(_abi.ctype("const char*")))
    assert _abi.ctype("const char*") is _abi.ctype("char*") is ctypes.c_char_p and _abi.ctype("void* const*") is ctypes.c_void_p
    assert len(consts) >= 22
    for name, value in consts.items():
        assert name.startswith("OSSID_") and getattr(hiplib, name[len("OSSID_"):]) == value, name
        checks += '_Static_assert(%s == %d, "%s");\n' % (name, value, name)
    assert sorted(consts) == sorted(set(re.findall(r"#define\s+(OSSID_\w+)[ \t]+\S", _header())))
    rc, err = _gcc(tmp_path, "protos.c", "void check(void) {\n%s}\n" % checks, "-c", "-o", str(tmp_path / "protos.o"))
    assert rc == 0, err
    # ... and the compile does refuse a table that is off by one swap: radius and nsample of the ball query
    ret, params = protos["ossid_pn2_ball_query"]
    swapped = params[:6] + [params[7], params[6]] + params[8:]
    assert swapped != params
    rc, err = _gcc(tmp_path, "swapped.c", "void check(void) {\n%s}\n" % _prototype_checks({"ossid_pn2_ball_query": (ret, swapped)}),
                   "-c", "-o", str(tmp_path / "swapped.o"))
    assert rc != 0 and "ossid_pn2_ball_query" in err
    # the binding: the table is the reader's, and every function of the loaded library carries its row
    handle = hiplib.lib()
    for name, (ret, params) in protos.items():
        assert hiplib._PROTOS[name] == (_abi.ctype(ret), [_abi.ctype(t) for t in params])
        f = getattr(handle, name)
        assert (f.restype, list(f.argtypes)) == hiplib._PROTOS[name], name


@pytest.mark.parametrize("text, names", [
    ("unsigned short ossid_f(int a);", "unsigned short"),                                      # a scalar outside the table
    ("int ossid_f(unsigned short a);", "unsigned short"),
    ("typedef struct ossid_s { int32_t a; void (*cb)(int); } ossid_s;", "cb"),                  # a function-pointer field
    ("typedef struct ossid_s { ossid_t b; } ossid_s;", "ossid_t"),                              # a type nobody declared
    ("int ossid_f(const float* x, ossid_t);", "ossid_t"),                                        # unnamed, unclassifiable
    ("int ossid_f(int, float y);", "int, float y"),                                             # unnamed
    ("typedef struct ossid_s { uint64_t a[OSSID_UNDEFINED]; } ossid_s;", "OSSID_UNDEFINED"),   # array sized by no #define
    ("#define OSSID_N (1 << 4)", "OSSID_N"),                                                   # not an integer literal
    ("#if OSSID_X\nint ossid_f(void);\n#endif", "#if"),
    ("int ossid_f(void)", "ossid_f"),                                                           # the ';' is missing ...
    ("int ossid_f(void) int ossid_g(void);", "ossid_g"),                                        # ... between two
    ("int ossid_f(void); int ossid_f(void);", "ossid_f"),
    ("int ossid_f();", "ossid_f"),
    ("const ossid_s* ossid_f(void);", "ossid_s"),
    ("int ossid_table[4];", "ossid_table"),
])
def test_header_reader_refuses_what_it_cannot_classify(text, names):
    from ossid_code_amd import _abi
    with pytest.raises(ValueError, match=re.escape(names)):
        _abi.parse(text)


def test_header_reader_reads_the_forms_the_header_uses():
    from ossid_code_amd import _abi
    consts, structs, protos = _abi.parse(
        "#ifndef OSSID_HIP_H\n#define OSSID_HIP_H\n#include <stdint.h>\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
        "#define OSSID_N 3 /* ossid_foo( */\n#define OSSID_E (-22)\n"
        "// int ossid_foo(int a);\n/* int ossid_foo(\n int a); */\n"
        "typedef struct ossid_s {\n const float* p; /* ossid_foo( */\n int32_t a, b[OSSID_N], c[2]; // d;\n void* const* q;\n} ossid_s;\n"
        "const char* ossid_names(void);\nvoid ossid_g(const ossid_s *s,\n   long  long n, char* out_host);\n"
        "#ifdef __cplusplus\n}\n#endif\n#endif /* OSSID_HIP_H */\n")
    assert consts == {"OSSID_N": 3, "OSSID_E": -22}
    assert structs == {"ossid_s": [("p", "const float*", 0), ("a", "int32_t", 0), ("b", "int32_t", 3), ("c", "int32_t", 2),
                                   ("q", "void* const*", 0)]}
    assert protos == {"ossid_names": ("const char*", []), "ossid_g": ("void", ["const ossid_s*", "long long", "char*"])}
    assert [_abi.ctype(t) for t in ("const ossid_s*", "long long", "char*", "void")] == \
        [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_char_p, None]


def test_no_cpu_fallback():
    """The product path refuses CPU tensors instead of silently computing elsewhere."""
    import torch
    from ossid_code_amd.zephyr import PointNet2SSG
    m = PointNet2SSG(8).eval()
    with pytest.raises(RuntimeError):
        m({"point_x": torch.zeros(1, 600, 8)})


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "ossid_code_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "zephyr_oracle" not in \
                    src.replace("oracle/zephyr_oracle.c", ""), f


def test_compat_install_resolves_reference_import_paths():
    """The names scripts/online_learning.py imports for the hot path resolve to this package after install()."""
    import subprocess
    import sys
    code = ("import ossid_code_amd.compat as c; c.install();"
            "from zephyr.datasets.score_dataset import ScoreDataset;"
            "from zephyr.models.pointnet2 import PointNet2SSG;"
            "from zephyr.options import getOptions;"
            "from zephyr.utils import K2meta, projectPointsUv;"
            "from ossid.utils.zephyr_utils import networkInference;"
            "from ossid.models.dtoid import DtoidNet;"
            "a = getOptions().parse_args([]); a.dataset='HSVD_diff_uv_norm'; a.no_valid_proj=True; a.no_valid_depth=True;"
            "d = ScoreDataset([], '', 'lmo', a, mode='test'); assert d.dim_point == 8;"
            "m = PointNet2SSG(d.dim_point, a, num_class=1); print('ok', DtoidNet.__module__, networkInference.__module__)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "ok ossid_code_amd.dtoid.model ossid_code_amd.scoring" in out.stdout


def test_seq_replay_passes_every_argument_class_through_the_c_loop(hiplib):
    """ossid_seq_replay (csrc/seq.hip) re-issues recorded calls through ONE call shape: integer-class arguments beyond the
    sixth and the stream on the stack, floats and doubles in xmm registers, negative 32-bit values, NULL. The probe entry
    point writes back what it received; the same ops through the Python loop must agree."""
    import ctypes as C
    lib = hiplib.lib()

    class FakeStream:
        def __init__(self, h):
            self.cuda_stream = h

        def wait_stream(self, other):
            pass
    out = [(C.c_double * 15)(), (C.c_double * 15)()]
    anchor = C.create_string_buffer(64)
    args = lambda o: (-7, 0.1, anchor, 1e300, -(1 << 40), 2 ** 31 - 1, -2.5, (1 << 63) + 5, -1, -123456, 77, -3.25e-7, 0, 1 << 50, o)
    for use_c, o in ((True, out[0]), (False, out[1])):
        seq = hiplib.Seq()
        seq.ops.append((lib.ossid_seq_probe, args(o), 1, "ossid_seq_probe"))
        seq.ops.append(("wait", 0, 0))                     # same stream on both sides: nothing to do, no HIP call
        seq.ops.append((lib.ossid_fill_zero, (None, 0), 0, "ossid_fill_zero"))     # zero bytes: returns before any HIP call
        old = hiplib.SEQ_C
        hiplib.SEQ_C = use_c
        try:
            seq.run((FakeStream(0x1000), FakeStream(0xABCDEF0123)))
            assert (seq._compiled is not None) == use_c
        finally:
            hiplib.SEQ_C = old
    want = [-7, float(C.c_float(0.1).value), C.addressof(anchor), 1e300, -(1 << 40), 2 ** 31 - 1, -2.5, float((1 << 63) + 5), -1,
            -123456, 77, -3.25e-7, 0, float(1 << 50), float(0xABCDEF0123)]
    assert list(out[0]) == want
    assert list(out[1]) == want
    # a failing op reports its status and index
    seq = hiplib.Seq()
    seq.ops.append((lib.ossid_fill_zero, (None, 0), 0, "ossid_fill_zero"))
    seq.ops.append((lib.ossid_fill_zero, (None, 8), 0, "ossid_fill_zero"))          # NULL with bytes: OSSID_EINVAL
    with pytest.raises(RuntimeError, match="ossid_fill_zero failed with status -22 .*op 1"):
        seq.run((FakeStream(0),))
