"""The C-ABI library loads and exports every entry point include/*.h declares
(CPU-only: no kernel is launched)."""
import ctypes
import glob
import os
import re

import pytest

from conftest import REPO

DECL = re.compile(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b([a-z][a-z0-9_]*)\s*\(", re.M)


def declared_symbols():
    names = set()
    for h in glob.glob(os.path.join(REPO, "include", "*.h")):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"//.*", "", txt)
        body = txt.split('extern "C" {', 1)[-1]
        for m in DECL.finditer(body):
            name = m.group(1)
            if name.startswith(("s3", "gsr", "s3n", "s3t")):
                names.add(name)
    return names


def test_headers_declare_entry_points():
    names = declared_symbols()
    assert "s3m_iter_proj" in names and "s3lie_sim3_act" in names
    assert len(names) >= 20


def test_library_exports_every_declared_symbol():
    from splatt3r_amd import _lib
    lib = _lib.lib()
    missing = [n for n in sorted(declared_symbols()) if not hasattr(lib, n)]
    assert not missing, f"declared but not exported: {missing}"


def test_every_declared_symbol_has_a_ctypes_signature():
    """Every name the regex above finds is a function the header parser found
    (splatt3r_amd/_abi.py), and so is bound when the library loads."""
    from splatt3r_amd import _abi, _lib
    missing = [n for n in sorted(declared_symbols()) if n not in _abi.functions]
    assert not missing, f"no ctypes signature for: {missing}"
    assert _lib.SIGNATURES.keys() == _abi.functions.keys()


def declared_param_counts():
    counts = {}
    for h in glob.glob(os.path.join(REPO, "include", "*.h")):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        txt = re.sub(r"//.*", "", txt)
        body = txt.split('extern "C" {', 1)[-1]
        for m in re.finditer(r"\b([a-z][a-z0-9_]*)\s*\(([^;{]*?)\)\s*;", body, flags=re.S):
            name, params = m.group(1), m.group(2).strip()
            if not name.startswith(("s3", "gsr")):
                continue
            counts[name] = 0 if params in ("", "void") else params.count(",") + 1
    return counts


def test_ctypes_signatures_match_header_arity():
    """Every ctypes argtypes list has exactly as many entries as the C
    declaration has parameters, counted by the independent regex above."""
    from splatt3r_amd import _abi
    counts = declared_param_counts()
    assert counts.keys() == _abi.functions.keys()
    bad = {n: (len(_abi.functions[n][1]), c) for n, c in counts.items()
           if len(_abi.functions[n][1]) != c}
    assert not bad, f"argtypes arity (ctypes, header) mismatch: {bad}"


def test_abi_metadata():
    from splatt3r_amd import _lib
    lib = _lib.lib()
    assert lib.s3_abi_version() >= 1
    assert lib.s3_arch() == b"gfx950"
    assert lib.s3_last_error() == b""


def test_error_path_reports_message():
    from splatt3r_amd import _lib
    lib = _lib.lib()
    # negative count is rejected before any device work
    st = lib.s3lie_sim3_inv(None, None, -1, None)
    assert st == 1
    assert b"n < 0" in lib.s3_last_error()


# typedef in include/*.h -> the module-level name the package keeps for it
STRUCTS = {
    "s3n_gemm_args": ("splatt3r_amd.ops", "GemmArgs"),
    "s3n_attn_args": ("splatt3r_amd.ops", "AttnArgs"),
    "s3n_gemm_tile": ("splatt3r_amd.ops", "GemmTile"),
    "gsr_settings": ("diff_gaussian_rasterization", "_GsrSettings"),
    "s3w_map": ("splatt3r_amd.gaussian_map", "S3wMap"),
    "s3w_view": ("splatt3r_amd.splatt3r_utils", "S3wView"),
    "s3v_in": ("splatt3r_amd.compact", "S3vIn"),
    "s3v_out": ("splatt3r_amd.compact", "S3vOut"),
    "s3o_adam": ("splatt3r_amd.refine", "S3oAdam"),
    "s3d_params": ("splatt3r_amd.refine", "S3dParams"),
    "s3x_pose_adam": ("splatt3r_amd.refine", "S3xPoseAdam"),
}


def test_struct_layouts_match_the_c_headers(tmp_path):
    """Every generated ctypes.Structure has the size and the field offsets
    the C compiler gives its typedef: one C program over include/*.h, built
    with gcc, prints them all."""
    import importlib
    import subprocess
    from splatt3r_amd import _abi, ops
    assert set(_abi.structs) == set(STRUCTS)
    for name, (mod, attr) in STRUCTS.items():
        assert getattr(importlib.import_module(mod), attr) is _abi.structs[name], name
    want, prints = {}, []
    for name, st in _abi.structs.items():
        want[name] = ctypes.sizeof(st)
        prints.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in st._fields_:
            want[f"{name}.{field}"] = getattr(st, field).offset
            prints.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(REPO, "include", "*.h")))
    src = "#include <stdio.h>\n#include <stddef.h>\n"
    src += "".join(f'#include "{h}"\n' for h in headers) + "int main(void) {\n" + "\n".join(prints) + "\n  return 0;\n}\n"
    (tmp_path / "layout.c").write_text(src)
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert len(want) > 11 + 100          # 11 sizes and every field of every struct
    assert got == want
    # the three facts the GemmArgs-only version of this test held
    assert ctypes.sizeof(ops.GemmArgs) == got["s3n_gemm_args"]
    assert ops.GemmArgs.Bp.offset == got["s3n_gemm_args.Bp"]
    assert ops.GemmArgs.ld_tail.offset == got["s3n_gemm_args.ld_tail"]


def param_index(fn, param):
    """Position of the parameter named `param` in fn's declaration, found with
    the regex of declared_param_counts (not with the parser under test)."""
    for h in glob.glob(os.path.join(REPO, "include", "*.h")):
        txt = re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S))
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % fn, txt, flags=re.S)
        if m:
            names = [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]
            return names.index(param)
    raise KeyError(fn)


def test_mapping_rules_on_real_entry_points():
    """The type mapping, pinned where a wrong width or kind would corrupt
    arguments silently: doubles by value, a string return, struct pointers,
    size_t returns."""
    from splatt3r_amd import _abi, gaussian_map, ops
    F = _abi.functions
    query = F["s3k_query"][1]
    assert query[param_index("s3k_query", "cell")] is ctypes.c_double
    assert query[param_index("s3k_query", "max_dist")] is ctypes.c_double
    assert query[param_index("s3k_query", "grid_bytes")] is ctypes.c_size_t
    assert query[param_index("s3k_query", "n")] is ctypes.c_int64
    assert query[param_index("s3k_query", "nx")] is ctypes.c_int32
    assert query[param_index("s3k_query", "origin")] is ctypes.c_void_p
    assert F["s3v_merge"][1][param_index("s3v_merge", "voxel")] is ctypes.c_double
    assert F["s3k_grid_build"][1][param_index("s3k_grid_build", "cell")] is ctypes.c_double
    assert F["s3k_dist_stats"][1][param_index("s3k_dist_stats", "threshold")] is ctypes.c_double
    assert F["s3_last_error"] == (ctypes.c_char_p, [])
    assert F["s3n_gemm"] == (ctypes.c_int, [ctypes.POINTER(ops.GemmArgs), ctypes.c_void_p])
    assert F["s3w_map_append"][1][0] is ctypes.POINTER(gaussian_map.S3wMap)
    assert F["s3p_workspace_bytes"][0] is ctypes.c_size_t
    assert F["s3n_gemm_workspace_bytes"][0] is ctypes.c_size_t
    assert F["s3n_gemm_set_debug"][0] is None
    assert F["s3n_prng_fill"][1][2] is ctypes.c_uint64
    assert F["s3n_layernorm"][1][3] is ctypes.c_void_p       # const float* const*
    assert F["s3_stream_create"][1][2] is ctypes.c_void_p    # void**
    C = _abi.constants
    assert C["S3N_MAX_GROUPS"] == ops.G == 4 and C["S3K_MAX_CELLS"] == 1 << 27
    assert (C["S3N_ACT_NONE"], C["S3N_ACT_GELU"], C["S3N_ACT_RELU"]) == (0, 1, 2)
    assert (C["S3_OK"], C["S3_ERR_INVALID"], C["S3_ERR_HIP"], C["S3_ERR_WORKSPACE"]) == (0, 1, 2, 3)
    assert C["S3P_NSUMS"] == 5 and C["S3C_COND_MATCH"] == 4


def test_abi_module_imports_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys; import splatt3r_amd._abi as a; assert len(a.functions) > 100; "
            "assert 'torch' not in sys.modules and 'splatt3r_amd._lib' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True,
                   cwd=os.path.join(REPO, "splatt3r-slam_amd"))


# ------------------------------------------------ the parser, on small texts --
def parse(text):
    from splatt3r_amd import _abi
    h = _abi.Headers()
    h.parse(text, "t.h")
    return h


def test_parser_struct_fields():
    h = parse("#define N 3\n"
              "typedef struct {\n"
              "  int H, W, d_sh, stride;\n"             # multi-declarator
              "  const float* A[N];\n"                  # array sized by a macro
              "  float bg[2], eps;\n"                   # array sized by a literal
              "  uint64_t seed;\n"
              "  int64_t* n;\n"
              "} t_view;\n"
              "int use(const t_view* v, t_view** vs);\n")
    st = h.structs["t_view"]
    assert issubclass(st, ctypes.Structure) and st.__name__ == "t_view"
    assert st._fields_ == [("H", ctypes.c_int), ("W", ctypes.c_int), ("d_sh", ctypes.c_int),
                          ("stride", ctypes.c_int), ("A", ctypes.c_void_p * 3),
                          ("bg", ctypes.c_float * 2), ("eps", ctypes.c_float),
                          ("seed", ctypes.c_uint64), ("n", ctypes.c_void_p)]
    assert h.functions["use"] == (ctypes.c_int, [ctypes.POINTER(st), ctypes.c_void_p])


def test_parser_function_declarations():
    h = parse('#ifndef T_H\n#define T_H\n#include <stdint.h>\n'
              '#ifdef __cplusplus\nextern "C" {\n#endif\n'
              "typedef enum { T_OK = 0, T_BAD = 1 } t_status;\n"
              "const char* t_error(void);\n"                                   # (void)
              "void t_reset();\n"
              "t_status t_rows(const float* const* x, void** out, void* const* o16);\n"
              "size_t t_bytes(int64_t, const float*, unsigned long long* scores);\n"  # unnamed
              "int t_split(const float* q,   /* [m, 3] */\n"
              "            double cell,      // by value\n"
              "            int32_t nx, float T[8]);\n"                         # three lines
              "uint64_t t_seed ( uint32_t pass ) ;\n"
              '#ifdef __cplusplus\n}\n#endif\n#endif /* T_H */\n')
    V = ctypes.c_void_p
    assert h.functions == {
        "t_error": (ctypes.c_char_p, []),
        "t_reset": (None, []),
        "t_rows": (ctypes.c_int, [V, V, V]),                                   # pointer-to-pointer
        "t_bytes": (ctypes.c_size_t, [ctypes.c_int64, V, V]),
        "t_split": (ctypes.c_int, [V, ctypes.c_double, ctypes.c_int32, V]),
        "t_seed": (ctypes.c_uint64, [ctypes.c_uint32]),
    }
    assert h.constants == {"T_OK": 0, "T_BAD": 1}                              # T_H has no value
    assert not h.structs


def test_parser_constants():
    h = parse("#define A 4\n#define B (1 << 27)\n#define C 0x10\n#define D (A << 2)\n"
              "#define F 1.5f\n#define M(x) (x)\n"
              "enum { P0, P1, P5 = 5, P6, PA = A, PB };\n"
              "typedef enum named { Q0 = 1, Q1 = 2,\n  Q2 = 4 } q_bits;\n"
              "q_bits get(q_bits* out);\n")
    assert h.constants == {"A": 4, "B": 1 << 27, "C": 16, "D": 16, "P0": 0, "P1": 1, "P5": 5,
                           "P6": 6, "PA": 4, "PB": 5, "Q0": 1, "Q1": 2, "Q2": 4}
    assert h.functions["get"] == (ctypes.c_int, [ctypes.c_void_p])


def test_parser_accepts_a_repeated_identical_declaration():
    h = parse("int f(int a, float* b);\nint f(int x,\n      float* y);\n")
    assert h.functions == {"f": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p])}


REJECTED = {
    "unknown type word": "int f(int a);\n\nint g(long a);\n",
    "unknown return type": "\n\nbool g(int a);\n",
    "unknown field type": "typedef struct {\n  int a;\n  short b;\n} s;\n",
    "struct by value": "typedef struct { int a; } s;\n\nint g(s v);\n",
    "struct returned by value": "typedef struct { int a; } s;\n\ns g(void);\n",
    "void by value": "\n\nint g(void a, int b);\n",
    "variadic": "\n\nint g(const char* fmt, ...);\n",
    "function pointer": "\n\nint g(void (*cb)(int), void* user);\n",
    "declared twice differently": "int g(float a);\n\nint g(double a);\n",
    "array of unknown size": "typedef struct {\n  int a;\n  float b[N];\n} s;\n",
    "pointer in a multi-declarator": "typedef struct {\n  int a;\n  float *b, c;\n} s;\n",
    "a definition": "\n\nint g(int a) { return a; }\n",
    "a tagged struct without typedef": "\n\nstruct s { int a; };\n",
    "a plain typedef": "\n\ntypedef int t_int;\n",
}


@pytest.mark.parametrize("what", list(REJECTED))
def test_parser_rejects(what):
    """Outside the vocabulary nothing is guessed: a ValueError names the
    header and the line.  Every text above has its fault in the statement
    that starts on line 3 (in a struct: the field on line 3)."""
    with pytest.raises(ValueError, match=r"^t\.h:3: ") as e:
        parse(REJECTED[what])
    print(e.value)


def test_shipped_library_has_no_packed_fp32_instructions(tmp_path):
    """Every kernel is built without v_pk_{mul,add,fma}_f32 (csrc/build.py
    NO_PACKED_FP32): on the MI355X boxes those return wrong values while
    MFMAs of another kernel run on the same CU (a GEMM on another stream
    corrupted 30-93 % of the matching kernels' launches,
    tools/stress_bd_concurrency.py).  Checked on the library that ships:
    every device bundle of its .hip_fatbin section is disassembled."""
    import shutil
    import subprocess
    import pytest
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler",
                                              "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not found")
    lib = os.path.join(REPO, "splatt3r-slam_amd", "splatt3r_amd", "_native", "libsplatt3r_hip.so")
    fat = tmp_path / "fatbin.bin"
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fat}", lib, str(tmp_path / "copy.so")],
                   check=True, capture_output=True)
    blob = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    offs = [m.start() for m in re.finditer(re.escape(magic), blob)]
    assert len(offs) >= 10, offs
    packed, disassembled = 0, 0
    for k, o in enumerate(offs):
        part = tmp_path / f"b{k}.bin"
        part.write_bytes(blob[o:offs[k + 1] if k + 1 < len(offs) else len(blob)])
        co = tmp_path / f"d{k}.co"
        r = subprocess.run([tools[1], "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}",
                            f"--output={co}"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        d = subprocess.run([tools[2], "-d", str(co)], capture_output=True, text=True).stdout
        disassembled += d.count("\n")
        packed += len(re.findall(r"\bv_pk_(?:mul|add|fma)_f32", d))
    shutil.rmtree(tmp_path, ignore_errors=True)
    assert disassembled > 100000
    assert packed == 0
