"""CPU-side checks of the drop-in boundary: libedtr_hip.so builds for gfx950, loads, and exports every entry point
declared in include/edtr_hip.h; the ctypes binding that edtr_amd/lib.py derives from that header (structs, constants,
prototypes) agrees with what the C compiler makes of the same file, and the reader refuses what it does not understand.  No
compute call is made (no GPU in the build container)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "edtr_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(edtr_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    from edtr_amd.build import build_library
    from edtr_amd import lib
    path = build_library()
    assert os.path.exists(path)
    handle = lib.load()
    names = declared_functions()
    assert len(names) >= 20
    for name in names:
        assert hasattr(handle, name), f"{name} declared in edtr_hip.h but not exported"
    assert sorted(lib.DECLARED_SYMBOLS) == names, "lib.DECLARED_SYMBOLS out of sync with the header"
    assert handle.edtr_abi_version() == 10
    assert b"EDTR_E_ALIGN" in handle.edtr_error_string(-3)
    assert handle.edtr_igemm(None, None) == -1          # NULL params -> EDTR_E_NULL, nothing launched


CNAME = {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t", ctypes.c_float: "float", ctypes.c_void_p: "void*"}


def gcc(tmp_path, name, body, *flags, run=True):
    """Compile `body` behind the header's #include; the program's stdout as {key: int} when it is run."""
    src = tmp_path / f"{name}.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edtr_hip.h"\n' + body)
    exe = tmp_path / name
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), *flags, str(src), "-o", str(exe)], capture_output=True, text=True)
    if not run:
        return r
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_ctypes_structs_match_the_c_layout(tmp_path):
    """sizeof of every struct of the header and offsetof of EVERY field, by the C compiler, against the derived ctypes classes."""
    from edtr_amd import lib
    assert len(lib.HEADER.structs) == 12 and sum(len(f) for f in lib.HEADER.structs.values()) > 200
    lines = []
    for c, fields in lib.HEADER.structs.items():
        lines.append(f'printf("{c} %zu\\n", sizeof({c}));')
        lines += [f'printf("{c}.{f} %zu\\n", offsetof({c}, {f}));' for f, _ in fields]
    got = gcc(tmp_path, "layout", "int main(void){" + "\n".join(lines) + "return 0;}\n")
    want = {}
    for py, c in lib.STRUCT_NAMES.items():
        cls = getattr(lib, py)
        assert [f for f, _ in cls._fields_] == [f for f, _ in lib.HEADER.structs[c]]
        want[c] = ctypes.sizeof(cls)
        want.update({f"{c}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    assert got == want
    assert got["edtr_ffn_params"] == ctypes.sizeof(lib.FfnParams) and got["edtr_lin320_params.gn_table"] == lib.Lin320Params.gn_table.offset


def test_constants_match_the_c_preprocessor(tmp_path):
    """Every EDTR_* macro the preprocessor knows after the header and every enumerator, evaluated by the compiler, against lib.NAME."""
    from edtr_amd import lib
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-dM", "-E", "-include", "edtr_hip.h", "-x", "c", os.devnull],
                       check=True, capture_output=True, text=True)
    macros = {line.split()[1] for line in r.stdout.splitlines() if line.startswith("#define EDTR_")} - {"EDTR_HIP_H"}
    consts = lib.HEADER.constants
    assert macros and macros <= set(consts)
    enumerators = set(consts) - macros
    assert {"EDTR_BF16", "EDTR_E_UNSUPPORTED", "EDTR_ACT_LRELU", "EDTR_ATTN_V3"} <= enumerators and len(enumerators) == 6 + 6 + 5 + 5
    got = gcc(tmp_path, "consts", "int main(void){" + "\n".join(f'printf("{n} %lld\\n", (long long)({n}));' for n in consts) + "return 0;}\n")
    assert got == consts
    for name, value in consts.items():
        assert getattr(lib, name[len("EDTR_"):]) == value
    assert (lib.ABI_VERSION, lib.COCO_ACC_MAX_ROWS, lib.CLS_FD_MAX_ELEMS, lib.E_ALIGN, lib.NOISE_SAMPLE_ROI) == (10, 1 << 22, 1 << 28, -3, 9)


def prototype_checks(lib, swap=None):
    """`ret (*chk_i)(T1, ..., Tn) = name;` per function: scalars spelled from the ctypes model, pointers as the header has them."""
    lines = []
    for i, name in enumerate(lib.DECLARED_SYMBOLS):
        restype, argtypes = lib.prototype(name)
        ret, params = lib.HEADER.functions[name]
        assert len(argtypes) == len(params)
        if swap and name == swap[0]:
            argtypes[swap[1]] = swap[2]
        args = [t.c if t.ptr else CNAME[a] for a, (_, t) in zip(argtypes, params)]
        lines.append(f"{ret.c if ret.ptr else CNAME[restype]} (*chk_{i})({', '.join(args) or 'void'}) = {name};")
    return "\n".join(lines) + "\n"


def test_prototypes_match_the_c_compiler(tmp_path):
    """A wrong width, a lost parameter or a shifted position in the derived argtypes is a compile error; so that the check is
    known to bite, one deliberately wrong width and one dropped parameter must fail to compile."""
    from edtr_amd import lib
    flags = ("-c", "-Werror=incompatible-pointer-types", "-Wall", "-Werror")        # -c: the initialisers are checked, nothing is linked
    assert len(lib.DECLARED_SYMBOLS) == len(declared_functions()) > 100
    r = gcc(tmp_path, "protos", prototype_checks(lib), *flags, run=False)
    assert r.returncode == 0, r.stderr[-3000:]
    assert lib.prototype("edtr_zero_bytes")[1] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert lib.prototype("edtr_coco_accumulate_workspace")[0] is ctypes.c_int64 and lib.prototype("edtr_error_string")[0] is ctypes.c_char_p
    bad = gcc(tmp_path, "bad_width", prototype_checks(lib, swap=("edtr_zero_bytes", 1, ctypes.c_int32)), *flags, run=False)
    assert bad.returncode != 0 and "chk_" in bad.stderr
    dropped = prototype_checks(lib).replace("(void*, int64_t, void*) = edtr_zero_bytes;", "(void*, void*) = edtr_zero_bytes;")
    assert dropped != prototype_checks(lib) and gcc(tmp_path, "bad_count", dropped, *flags, run=False).returncode != 0


def test_struct_pointers_and_the_device_copy_rule():
    """descs_host is POINTER(Struct), the descs that follows it is the device copy and c_void_p; no other struct pointer is c_void_p."""
    from edtr_amd import lib
    device_copies = []
    for name, (_, params) in lib.HEADER.functions.items():
        for (pname, t), a in zip(params, lib.prototype(name)[1]):
            if t.base in lib.STRUCTS:
                if a is ctypes.c_void_p:
                    device_copies.append((name, pname))
                else:
                    assert a is ctypes.POINTER(lib.STRUCTS[t.base]), (name, pname)
    assert device_copies == [("edtr_image_resize_h_batch", "descs"), ("edtr_image_resize_ingest_batch", "descs"), ("edtr_det_transform", "descs")]
    P = ctypes.POINTER
    assert lib.prototype("edtr_image_resize_h_batch")[1][:2] == [P(lib.ImageDesc), ctypes.c_void_p]
    assert lib.prototype("edtr_image_resize_ingest_batch")[1][:2] == [P(lib.ImageDesc), ctypes.c_void_p]
    assert lib.prototype("edtr_det_transform")[1][:2] == [P(lib.DetImage), ctypes.c_void_p]
    assert lib.prototype("edtr_swin_layer")[1] == [P(lib.SwinAttnParams), P(lib.SwinMlpParams), ctypes.c_void_p]


GOOD = "typedef struct edtr_p { int32_t a, b; const float* x; } edtr_p;\nint edtr_f(const edtr_p* p,\n           edtr_stream_t stream);\n"


@pytest.mark.parametrize("text, line", [
    ("typedef struct edtr_q {\n    int32_t a;\n    unsigned flags;\n} edtr_q;\n", "unsigned flags"),
    ("typedef struct edtr_q {\n    int32_t a;\n    float w[4];\n} edtr_q;\n", "float w[4]"),
    ("int edtr_g(int n, int (*done)(void* ctx), void* ctx);\n", "int edtr_g(int n, int (*done)(void* ctx), void* ctx);"),
    ("int edtr_g(int n)\nint edtr_h(void);\n", "int edtr_g(int n)"),
    ("#define EDTR_SCALE 1.5f\n", "#define EDTR_SCALE 1.5f"),
    ("typedef struct edtr_q { int32_t a; struct { int32_t b; } in; } edtr_q;\n", "typedef struct edtr_q"),
    ("#define EDTR_N (1 << 4) + x\n", "#define EDTR_N (1 << 4) + x"),
    ("enum edtr_e { EDTR_A = 0, EDTR_B };\n", "EDTR_B"),
])
def test_the_header_reader_fails_closed(text, line):
    """Outside the header's dialect the reader raises and quotes the line: an `unsigned` field, an array field, a callback
    parameter, a prototype without its semicolon, a #define that is no integer expression (and a nested struct, a free name in
    an expression, an enumerator without a value)."""
    from edtr_amd import header
    h = header.parse(GOOD)
    assert list(h.functions) == ["edtr_f"] and [f for f, _ in h.structs["edtr_p"]] == ["a", "b", "x"]
    with pytest.raises(header.HeaderError) as e:
        header.parse(GOOD + text)
    assert line in str(e.value) and f"edtr_hip.h:{GOOD.count(chr(10)) + 1 + text.split(line)[0].count(chr(10))}:" in str(e.value)


def test_integer_expressions_are_evaluated_without_eval():
    from edtr_amd import header
    assert [header.int_expr(s) for s in ("10", " (1 << 22)", "-3", "((1<<2) << 1)", "1 << 2 << 3")] == [10, 1 << 22, -3, 8, 32]
    for bad in ("", "1 +", "(1 << 2", "__import__('os')", "1 << x", "0x10", "1.5", "2 2"):
        with pytest.raises(ValueError):
            header.int_expr(bad)


def test_the_binding_imports_neither_torch_nor_numpy():
    """tools/hipfree.py exists because `import torch` dominates a short run: edtr_amd.lib must stay importable without it, and
    hipfree (numpy is its own array type) must bind every entry point through lib.bind without pulling torch in."""
    from edtr_amd.build import build_library
    build_library()
    code = "import sys; import edtr_amd.lib as L; assert L.IgemmParams and L.BF16 == 0; print(sorted({'torch', 'numpy'} & set(sys.modules)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "[]", r.stdout + r.stderr[-2000:]
    code = ("import sys; sys.path.insert(0, 'tools'); import hipfree as H; assert H.DRY and H.edtr.edtr_layernorm.argtypes == H.L.prototype('edtr_layernorm')[1];"
            "assert H.edtr.edtr_igemm.argtypes[0] is H.C.POINTER(H.L.IgemmParams); print('torch' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, HIPFREE_DRY="1"))
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stdout + r.stderr[-2000:]


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from edtr_amd import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU/PyTorch fallback"):
        lib.load()


def test_no_kernel_spills_to_scratch():
    """Every gfx950 kernel of libedtr_hip.so keeps its state in registers / LDS: no scratch (private-segment) memory, no VGPR
    spills.  Round 4 found the 256x256 ping-pong kernel staging its 128 accumulators through 528 bytes of scratch per lane — a
    `#pragma unroll` loop around the shared epilogue had silently stopped unrolling when the epilogue grew — and nothing had
    looked.  Reads the code objects' notes (tools/kernel_resources.py); needs the ROCm LLVM tools, no GPU."""
    import importlib.util
    tool = os.path.join(ROOT, "tools", "kernel_resources.py")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("ROCm LLVM tools not installed")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    tail = r.stdout.strip().splitlines()[-1]
    assert tail.endswith(" 0 with scratch / spills"), r.stdout[-3000:]
    assert int(tail.split()[0]) >= 100, tail          # the library's kernels were actually enumerated
