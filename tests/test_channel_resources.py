"""Resources of the channel kernel on the detection path (uint8 images, shrink 2, smoothed), read from the gfx950 code
objects of the built library with the ROCm LLVM tools -- no GPU needed.  Five workgroups of 256 threads per CU need at
most 160 KiB / 5 = 32 KiB of LDS and 96 VGPRs per lane (no AGPRs, no spills): a change must not silently drop the
kernel back to four."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from waldboost_amd import _native as nat

KERNEL = "_ZN12_GLOBAL__N_115channels_kernelIhLi2ELi16ELi64ELb1ELb1ELi256EEEvNS_8ChanArgsE"
TARGET = b"hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _readelf():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for path in (os.path.join(rocm, "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf")):
        if path and os.access(path, os.X_OK):
            return path
    pytest.fail("llvm-readelf of the ROCm toolchain not found (set ROCM_PATH)")


def _gfx950_code_objects(blob):
    """The gfx950 entries of every offload bundle in the library (one bundle per translation unit): header = magic,
    entry count, then per entry offset, size, target-name length and name (little-endian uint64s)."""
    at = blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen]
            p += 24 + tlen
            if triple == TARGET:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + 1)


def _kernel_metadata(tmp_path, name):
    nat.load()
    blob = open(nat.LIB_PATH, "rb").read()
    for i, co in enumerate(_gfx950_code_objects(blob)):
        f = tmp_path / f"co{i}.elf"
        f.write_bytes(co)
        notes = subprocess.run([_readelf(), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
        # kernels are the items of the amdhsa.kernels list: "  - .agpr_count: ..." up to the next item
        for item in re.split(r"\n  - ", notes):
            if re.search(r"^\s*\.name:\s+" + re.escape(name) + r"\s*$", item, re.M):
                return dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", item, re.M))
    pytest.fail(f"{name} not found in the gfx950 code objects of {nat.LIB_PATH}")


def test_detection_channel_kernel_fits_five_workgroups_per_cu(tmp_path):
    md = _kernel_metadata(tmp_path, KERNEL)
    assert int(md["group_segment_fixed_size"]) <= 160 * 1024 // 5, md["group_segment_fixed_size"]
    assert int(md["vgpr_count"]) <= 96, md["vgpr_count"]
    assert int(md["agpr_count"]) == 0, md["agpr_count"]
    assert int(md["vgpr_spill_count"]) == 0, md["vgpr_spill_count"]
    assert int(md["private_segment_fixed_size"]) == 0, md["private_segment_fixed_size"]
