"""The C-ABI library builds, loads and exports every symbol include/*.h declares (no compute)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = set()
    for h in ("rtgs_raster.h", "rtgs_debug.h", "rtgs_icp.h", "rtgs_slam.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(rtgs_[a-z0-9_]+)\s*\(", src))
    names.discard("rtgs_resize_fn")
    return names


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from rtg_slam_amd import _lib
    lib = _lib.load()
    decl = declared_symbols()
    assert decl, "no declarations parsed"
    assert decl == set(_lib.EXPORTED_SYMBOLS)
    for name in decl:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.rtgs_version()


def test_product_path_has_no_oracle_or_cpu_fallback():
    for d in ("rtg_slam_amd", "diff_gaussian_rasterization_depth", "simple_knn", "cuda_utils"):
        for fn in os.listdir(os.path.join(ROOT, d)):
            if fn.endswith(".py"):
                src = open(os.path.join(ROOT, d, fn)).read()
                assert "import oracle" not in src and "from oracle" not in src, fn


def test_cpu_tensors_are_rejected_loudly():
    import pytest
    import torch
    from diff_gaussian_rasterization_depth import GaussianRasterizer
    from tests import raster_util as ru
    from rtg_slam_amd import synth
    cam = synth.CameraSpec(32, 32, 40.0, 40.0, 15.5, 15.5)
    g, s = ru.make_scene(10, cam)
    rast = GaussianRasterizer(raster_settings=ru.hip_settings(s, "cpu"))
    with pytest.raises(RuntimeError, match="HIP device"):
        rast(means3D=g["xyz"], opacities=g["opacity"], shs=g["shs"], colors_precomp=None, scales=g["scales"],
             rotations=g["rotations"], cov3D_precomp=None, normal_w=g["normal"], tile_mask=None)


HEADERS = ("rtgs_raster.h", "rtgs_debug.h", "rtgs_icp.h", "rtgs_slam.h")
STRUCTS = ("rtgs_raster_settings", "rtgs_loss_signs", "rtgs_attach", "rtgs_activated", "rtgs_loss_cfg", "rtgs_map_step_args",
           "rtgs_icp_level")


def declared_members():
    """struct name -> member names in order, by this test's own reading of the headers (every word in front of a , or ;)."""
    out = {}
    for h in HEADERS:
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", src, flags=re.S):
            out[name] = re.findall(r"(\w+)\s*[,;]", body)
    return out


def test_struct_layouts_match_the_host_compiler(tmp_path):
    """sizeof, and offsetof / sizeof of every member, of all seven structs as a C compiler lays them out against the ctypes
    classes the binding derives from the headers."""
    import ctypes as C
    import shutil
    import subprocess
    from rtg_slam_amd import _lib
    members = declared_members()
    assert set(members) == set(STRUCTS) == set(_lib.STRUCTS)
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{h}"' for h in HEADERS] + ["int main(void) {"]
    for s in STRUCTS:
        lines.append(f'  printf("{s} - %zu 0\\n", sizeof({s}));')
        lines += [f'  printf("{s} {m} %zu %zu\\n", offsetof({s}, {m}), sizeof((({s}*)0)->{m}));' for m in members[s]]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    compiled = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    got = [tuple(l.split()) for l in compiled if l]
    want = []
    for s in STRUCTS:
        cls = _lib.STRUCTS[s]
        assert [n for n, _ in cls._fields_] == members[s], s
        want.append((s, "-", str(C.sizeof(cls)), "0"))
        want += [(s, n, str(getattr(cls, n).offset), str(getattr(cls, n).size)) for n, _ in cls._fields_]
    assert got == want
    assert [C.sizeof(_lib.STRUCTS[s]) for s in STRUCTS] == [104, 32, 24, 32, 32, 528, 48]
    for alias, s in (("RasterSettingsC", "rtgs_raster_settings"), ("IcpLevelC", "rtgs_icp_level"), ("LossCfgC", "rtgs_loss_cfg"),
                     ("AttachC", "rtgs_attach"), ("ActivatedC", "rtgs_activated"), ("MapStepArgsC", "rtgs_map_step_args")):
        assert getattr(_lib, alias) is _lib.STRUCTS[s]


def test_derived_prototypes_of_a_few_functions():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from rtg_slam_amd import _lib
    lib = _lib.load()
    P, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    want = {
        "rtgs_slam_map_step_ctx": (C.c_int, [P, C.POINTER(_lib.MapStepArgsC), P, P]),
        "rtgs_map_tail_rows": (C.c_int, [P] * 23 + [i64, i32, f32, f32, f32, C.POINTER(_lib.AttachC), P, P,
                                                    C.POINTER(_lib.ActivatedC), P]),
        "rtgs_mesh_decimate_propose": (C.c_int, [P, P, i64, i64, P, P, P, P, C.c_double, P, P, P]),
        "rtgs_raster_set_map_epoch_ctx": (None, [P, C.c_uint64]),
        "rtgs_version": (C.c_char_p, []),
        "rtgs_ctx_create": (C.c_void_p, []),
        "rtgs_raster_forward": (C.c_int, [C.POINTER(_lib.RasterSettingsC), i32, i32] + [P] * 15
                                + [_lib.RESIZE_FN, P, _lib.RESIZE_FN, P, _lib.RESIZE_FN, P, P, P]),
    }
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is res, name
        assert list(fn.argtypes) == args, name
    assert _lib.RESIZE_FN._restype_ is C.c_void_p and tuple(_lib.RESIZE_FN._argtypes_) == (C.c_void_p, C.c_size_t)


def test_reader_refuses_what_it_does_not_understand():
    import pytest
    from rtg_slam_amd import _cdecl
    ok = _cdecl.Declarations().read("typedef struct rtgs_s { float *a, *b; int32_t n; } rtgs_s;\nint rtgs_f(const rtgs_s* s, void* stream);")
    assert [n for n, _ in ok.structs["rtgs_s"]._fields_] == ["a", "b", "n"] and len(ok.functions["rtgs_f"][1]) == 2
    for snippet in ("int rtgs_f(unsigned x);",                                        # an unknown type
                    "int rtgs_f(rtgs_t* x);",
                    "int rtgs_f(void* (*resize)(void* user, size_t bytes), void* stream);",   # a callback written inline
                    "typedef struct rtgs_s { int32_t a : 3; } rtgs_s;",               # a bit-field
                    "typedef struct rtgs_s { int32_t a[4]; } rtgs_s;",
                    "typedef struct rtgs_s { int32_t a;",                             # an unterminated struct
                    "#define RTGS_HALF 0.5",
                    "#if 0\n#endif"):
        with pytest.raises(_cdecl.CDeclError):
            _cdecl.Declarations().read(snippet)


def test_constants_come_from_the_headers():
    from rtg_slam_amd import _lib, icp, mesh_ops, meshing, evaluation
    assert (icp.FLAG_PERSISTENT, icp.FLAG_CLUSTER, icp.FLAG_SCRATCH_READY, icp.FLAG_FROM_IDENTITY, icp.FLAG_F32_SOLVE,
            icp.FLAG_LAST_ARRIVER) == (1, 2, 4, 8, 16, 32)
    assert (icp.PYR_SCRATCH_READY, icp.PYR_SECOND_SET) == (1, 2)
    assert mesh_ops.DISTANCE_MAX_DIM == 65536 and mesh_ops.MAX_CELLS == 1 << 21 and mesh_ops.REGISTER_OUT == 30
    assert meshing.BRICK_BYTES == 10240 and meshing.TEXTURE_MAX_SIDE == evaluation.MESH_TEXTURE_MAX_SIDE == 16384
    assert _lib.FWD_NO_BACKWARD == 1
    assert _lib.CONSTANTS["RTGS_E_INVALID"] == -1 and _lib.CONSTANTS["RTGS_TSDF_MAX_VOXELS"] == 2147483647     # (-1), ...LL


def test_ctypes_mirrors_match_the_c_structs():
    """Layout guard: the two structs that cross the C ABI have the size their ctypes mirrors have (also enforced at
    load time), and the optimiser's one-call step refuses CPU tensors like every other entry point."""
    import ctypes as C
    import pytest
    import torch
    from rtg_slam_amd import _lib, map_optim as mo
    lib = _lib.load()
    assert C.sizeof(_lib.MapStepArgsC) == lib.rtgs_map_step_args_size()
    assert C.sizeof(_lib.RasterSettingsC) == lib.rtgs_raster_settings_size()
    packed = torch.zeros(8, mo.COLS)
    opt = mo.ShardedMapOptimizer(packed)           # CPU tensors: no arena, HIP kernels unavailable
    assert opt.grad_rows is None
    with pytest.raises(RuntimeError, match="HIP device"):
        opt.step(lambda gd: gd["xyz"].sum())
