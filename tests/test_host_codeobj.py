"""CPU-side check of the BUILT library's gfx950 code objects: no packed fp32 VALU math.

csrc/Makefile builds every file without the packed-fp32-ops target feature because v_pk_fma_f32 miscomputes lanes 48-63 next to
other waves' 16-bit MFMAs on this hardware (profiles/micro/pk_fma_coexec.hip).  One cc1 flag is all that keeps those instructions
out, and a numeric test only rarely sees the fault, so this test reads the instructions themselves: it extracts the .hip_fatbin
section, splits it into the offload bundles the link concatenated (one per source file the Makefile compiles), unbundles the gfx950
code object of each and disassembles them all.
"""
import importlib
import os
import re
import shutil
import struct
import subprocess

import pytest

L = importlib.import_module("attention-gan_amd.backend.lib")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEFILE = os.path.join(ROOT, "attention-gan_amd", "csrc", "Makefile")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
PACKED_FP32 = ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32")


def _tool(name):
    path = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    if not os.access(path, os.X_OK):
        path = shutil.which(name)
    if not path:
        pytest.skip(f"{name} not found under $ROCM_PATH/llvm/bin or on PATH: cannot disassemble the code object")
    return path


def _makefile_sources():
    m = re.search(r"^SRCS\s*:=\s*(.+)$", open(MAKEFILE).read(), re.M)
    assert m, "no SRCS line in csrc/Makefile"
    return m.group(1).split()


def split_bundles(fatbin: bytes):
    """-> the offload bundles of a .hip_fatbin section, in order.  The linker concatenates one uncompressed bundle per object file,
    each padded to its alignment with zeros; a bundle's header (magic, entry count, then per entry: offset, size, triple length,
    triple) says where its last entry ends, and the next bundle starts at the next magic after that."""
    out, pos = [], 0
    while True:
        pos = fatbin.find(MAGIC, pos)
        if pos < 0:
            return out
        q = pos + len(MAGIC)
        n, = struct.unpack_from("<Q", fatbin, q)
        q += 8
        end = q
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, q)
            q += 24 + tlen
            end = max(end, pos + off + size)
        assert 0 < n < 64 and end <= len(fatbin), f"malformed offload bundle header at offset {pos}"
        out.append(fatbin[pos:end])
        pos = end


def _disassemble_all(lib_path, tmp_path):
    """-> list of (bundle index, disassembly of its gfx950 code object)"""
    objcopy, bundler, objdump = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-objdump")
    fatbin = tmp_path / "lib.hip_fatbin"
    # (--dump-section still writes the library's copy; send it to tmp_path so the tree is untouched)
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fatbin}", str(lib_path), str(tmp_path / "lib.copy")],
                   check=True, capture_output=True)
    out = []
    for i, bundle in enumerate(split_bundles(fatbin.read_bytes())):
        src, code = tmp_path / f"bundle{i}.bin", tmp_path / f"gfx950_{i}.co"
        src.write_bytes(bundle)
        subprocess.run([bundler, "--type=o", f"--targets={TARGET}", f"--input={src}", f"--output={code}", "--unbundle"],
                       check=True, capture_output=True)
        out.append((i, subprocess.run([objdump, "-d", str(code)], check=True, capture_output=True, text=True).stdout))
    return out


def test_code_object_has_no_packed_fp32_instructions(tmp_path):
    assert os.path.exists(L.LIB_PATH), f"{L.LIB_PATH} not built"
    objects = _disassemble_all(L.LIB_PATH, tmp_path)
    srcs = _makefile_sources()
    assert len(objects) == len(srcs), f"{len(objects)} gfx950 code objects in the library, the Makefile builds {len(srcs)} sources: extraction missed some"
    assert sum(len(re.findall(r"\bv_mfma", asm)) for _, asm in objects) > 0, "no v_mfma in the disassembly: the code objects were not extracted"
    found = {}
    for i, asm in objects:
        n = {op: len(re.findall(rf"\b{op}\b", asm)) for op in PACKED_FP32}
        if any(n.values()):
            found[f"{srcs[i]} (bundle {i})"] = n          # (the link concatenates the objects in SRCS order)
    assert not found, f"packed fp32 VALU instructions in the gfx950 code objects of {L.LIB_PATH}: {found}"
