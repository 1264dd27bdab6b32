"""The resource budget of the slim form of the 4-wave kernel (conv_mfma_f16x3_w4d_slim_kernel, conv_f16x3_w4d.h): three
blocks share a compute unit only while a block stays within a third of it -- 168 vector registers (512 / 3 waves per SIMD, in granules of 8), no
scratch memory, 54 528 B of LDS (163 840 / 3, down to a multiple of 128).  The registers and the private segment are read
from the built library's code object (its AMDGPU metadata note), the LDS from what the planner requests (the kernel has no
static LDS: the note says so).  No GPU is needed."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

from smallhardface_amd import _lib
from smallhardface_amd import build as B

VGPR_MAX = 168
LDS_MAX = 163840 // 3 // 128 * 128
# one halo buffer (4 planes of 10 rows x 24 pixels x 16 B, + 32 B), a ring of four tap slabs (128 couts x 64 B), 128 biases
LDS_SLIM = 4 * (10 * 24 * 16 + 32) + 4 * 128 * 64 + 128 * 4
# conv_mfma_f16x3_w4d_slim_kernel<IN_SPLIT, NP, BF>
SLIM_NAME = re.compile(r"conv_mfma_f16x3_w4d_slim_kernelILb[01]ELi[123]ELb[01]EEE")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    dirs = [os.path.join(os.path.dirname(p), "..", "llvm", "bin") for p in (B.HIPCC, os.path.realpath(B.HIPCC))]
    for d in dirs + ["/opt/rocm/llvm/bin"]:
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    found = shutil.which(name)
    assert found, "%s not found beside %s" % (name, B.HIPCC)
    return found


def _gfx950_code_objects(path):
    """The gfx950 code objects of every offload bundle in the library (one bundle per translation unit)."""
    blob = open(path, "rb").read()
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, pos)
            ident = blob[pos + 24:pos + 24 + idlen].decode()
            pos += 24 + idlen
            if B.ARCH in ident and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, at + len(MAGIC))
    return out


def _kernel_notes(path, tmp_path):
    """{kernel symbol: {metadata key: int}} over the library's gfx950 code objects (llvm-readelf --notes)."""
    kernels = {}
    for i, co in enumerate(_gfx950_code_objects(path)):
        f = tmp_path / ("co_%d.o" % i)
        f.write_bytes(co)
        txt = subprocess.run([_tool("llvm-readelf"), "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        cur, group = None, None
        for line in txt.splitlines():
            m = re.match(r"\s*(?:- )?\.(\w+):\s+(\S+)\s*$", line)
            if not m:
                continue
            key, val = m.group(1), m.group(2)
            if key == "group_segment_fixed_size":      # (the keys of a kernel come in alphabetical order: this one before .name)
                group = int(val)
            elif key == "name" and val.startswith("_Z"):
                cur = kernels.setdefault(val, {"group_segment_fixed_size": group})
            elif key == "wavefront_size":
                cur = None
            elif cur is not None and key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                             "agpr_count"):
                cur[key] = int(val)
    return kernels


def test_slim_kernels_fit_three_waves_per_simd(tmp_path):
    lib = _lib.load(require_gpu=False)
    assert lib is not None
    notes = _kernel_notes(_lib.LIB_PATH, tmp_path)
    assert len(notes) > 50, len(notes)                       # the note really was parsed
    slim = {k: v for k, v in notes.items() if SLIM_NAME.search(k)}
    assert len(slim) == 7, sorted(slim)                      # [IN_SPLIT x NP] + bf16
    for name, k in slim.items():
        print(name, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= VGPR_MAX, (name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)  # all of its LDS is what the planner requests
    # the two-per-CU form it stands beside is untouched by the bound (it needs its ~200 registers)
    fat = [v for k, v in notes.items() if re.search(r"w4d_kernelILb1ELi2ELi1ELi3ELb0ELi1EEE", k)]
    assert len(fat) == 1 and fat[0]["private_segment_fixed_size"] == 0


@pytest.mark.parametrize("in_split", [0, 1])
@pytest.mark.parametrize("pooled", [0, 1])
@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 128), (128, 256)])
def test_planner_requests_a_third_of_the_lds(cin, cout, pooled, in_split):
    lib = _lib.load(require_gpu=False)
    fn = lib.shf_debug_conv_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    assert LDS_SLIM == 48768 and LDS_SLIM <= LDS_MAX == 54528
    for h, w in ((8, 16), (9, 17), (23, 40), (256, 416)):
        lds, grid, slim = (C.c_longlong * 2)(), (C.c_longlong * 2)(), (C.c_int * 2)()
        nl = fn(cin, cout, h, w, in_split, pooled, lds, grid, slim)
        assert nl == 1, _lib.last_error()
        assert grid[0] == -(-h // 8) * -(-w // 16) * (cout // 128)       # single 8-row tiles x cout tiles
        if os.environ.get("SHF_F16X3_W4_SLIM", "1") != "0":
            assert slim[0] == 1 and lds[0] == LDS_SLIM <= LDS_MAX, (lds[0], slim[0])
        else:
            assert slim[0] == 0 and lds[0] == 2 * 15488 + 2 * 3 * 8192 + 512
    # deeper layers are not its business
    nl = fn(256, 256, 64, 64, in_split, pooled, lds, grid, slim)
    assert nl >= 1 and not any(slim[i] for i in range(nl))
