"""The cascade tile per form, without a GPU: wb_model_geometry (what wb_model_create chooses), the LDS layout of
wb_cascade_tile.h mirrored here, the constants the generator of the specialised kernel writes into its prelude, and the
registers of the specialised 64-row build, read from its code object with the ROCm LLVM tools.

The one-byte forms (uint8 channels, 8-bit ranks) scan 64 x 64 windows per workgroup where 40 KB of LDS hold that tile --
four workgroups per CU, and eight waves per SIMD need at most 64 VGPRs per lane; the float32 and the two-byte form keep
32 rows."""
import ctypes as C
import re
import subprocess

import pytest

from test_channel_resources import _readelf
from waldboost_amd import _native as nat

FORMS = {"f32": (nat.WB_DTYPE_F32, 0), "u8": (nat.WB_DTYPE_U8, 1), "rank8": (nat.WB_DTYPE_RANK8, 1), "rank16": (nat.WB_DTYPE_RANK16, 2)}
STAGE_DWORDS = {d: (2 * (2 ** d - 1) + 2 ** d + 1 + 3) // 4 * 4 for d in (1, 2, 3)}      # WB_STAGE_DWORDS


def geometry(T, depth, shape, form):
    out = (C.c_int32 * 4)()
    nat.check(nat.load().wb_model_geometry(T, depth, *shape, FORMS[form][0], out), "wb_model_geometry")
    return tuple(out)                                      # rows per wave, waves, tile rows, LDS bytes


def lds_bytes(T, depth, shape, eb, tile_rows, waves):
    """wb_cascade_tile.h: [ tile | queue | hist | (16-aligned) stage mirror | 256 B of control words ]"""
    m, n, Cc = shape
    rows, pitch = tile_rows + m - 1, 64 + n
    tile = (Cc * rows * pitch * eb + 15) // 16 * 16 if eb else Cc * rows * pitch * 4
    qcap = min(tile_rows * 64, 64 * waves + (768 if tile_rows > 32 else 512))
    mirror = T if T * STAGE_DWORDS[depth] * 4 <= 16 * 1024 else 0
    return (tile + qcap * 8 + T * 4 + 15) // 16 * 16 + mirror * STAGE_DWORDS[depth] * 4 + 256


@pytest.mark.parametrize("T,depth,shape", [(128, 2, (12, 12, 4)), (256, 2, (12, 12, 4)), (24, 2, (12, 12, 4)), (40, 3, (12, 12, 4)),
                                           (32, 1, (16, 16, 4)), (128, 2, (24, 24, 4)), (128, 2, (12, 12, 3))])
def test_tile_rows_and_lds_per_form(T, depth, shape):
    rpw, waves, rows, lds = geometry(T, depth, shape, "f32")
    assert rows == rpw * waves and lds == lds_bytes(T, depth, shape, 0, rows, waves)
    for form in ("rank16", "u8", "rank8"):
        eb = FORMS[form][1]
        f_rpw, f_waves, f_rows, f_lds = geometry(T, depth, shape, form)
        assert f_waves == waves and f_rows == f_rpw * f_waves and f_lds == lds_bytes(T, depth, shape, eb, f_rows, waves), form
        tall = eb == 1 and (rpw, waves) == (4, 8) and lds_bytes(T, depth, shape, 1, 64, 8) <= 40960
        assert f_rows == (64 if tall else rows), form      # (a multiple of the model's rows: the unit of the tile table)
        assert not tall or f_lds <= 40960


def test_the_benchmark_shapes_get_the_tall_tile():
    """128 stages of depth 2 on 12 x 12 x 4 windows: 64 rows in under 40 KB on the one-byte forms.  256 stages: the
    mirror is 6 KB larger and the tile stays at 32 rows."""
    assert geometry(128, 2, (12, 12, 4), "rank8")[2:] == (64, 39952)
    assert geometry(128, 2, (12, 12, 4), "f32")[2] == geometry(128, 2, (12, 12, 4), "rank16")[2] == 32
    assert geometry(256, 2, (12, 12, 4), "rank8")[2] == 32 and lds_bytes(256, 2, (12, 12, 4), 1, 64, 8) > 40960


def test_specialised_tall_build_prelude_and_registers(tmp_path, monkeypatch):
    """wb_jit_compile_check3 builds the specialised kernel of a synthetic 128-stage depth-2 cascade on 12 x 12 x 4 windows
    at eight rows per wave; WB_JIT_DUMP_DIR keeps its source and code object."""
    monkeypatch.setenv("WB_JIT_DUMP_DIR", str(tmp_path))
    rpw, waves, rows, _ = geometry(128, 2, (12, 12, 4), "rank8")
    n = C.c_int64()
    nat.check(nat.load().wb_jit_compile_check3(2, 128, 1, rpw, b"gfx950", C.byref(n)), "wb_jit_compile_check3")
    src = (tmp_path / "wb_casc_jit.hip").read_text()
    defs = {k: int(v) for k, v in re.findall(r"^#define (WB_JIT_(?:RPW|WAVES|ROWS|PITCH|C|T|LDS_STAGES)) (\d+)$", src, re.M)}
    assert defs == dict(WB_JIT_RPW=rpw, WB_JIT_WAVES=waves, WB_JIT_ROWS=rows + 11, WB_JIT_PITCH=76, WB_JIT_C=4, WB_JIT_T=128, WB_JIT_LDS_STAGES=128)
    assert f"cascade_tile_body<2, {rpw}, {waves}, 1, true>" in src
    notes = subprocess.run([_readelf(), "--notes", str(tmp_path / "wb_casc_jit.co")], check=True, capture_output=True, text=True).stdout
    md = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", notes, re.M))
    assert int(md["vgpr_count"]) <= 64, md["vgpr_count"]
    assert int(md.get("agpr_count", 0)) == 0 and int(md["vgpr_spill_count"]) == 0 and int(md["private_segment_fixed_size"]) == 0, md


def test_tuning_overrides_reach_64_rows_on_the_byte_forms_only(monkeypatch):
    """WB_CASC_RPW=8 WB_CASC_WAVES=8: the float32 budget halves the model's rows per wave back to 4, the one-byte forms
    take the 8 asked for.  WB_CASC_RPW=4 (or WB_CASC_BYTE_RPW=4): 32 rows everywhere.  2 rows per wave: 16 and 16."""
    shape = (12, 12, 4)
    monkeypatch.setenv("WB_CASC_RPW", "8")
    monkeypatch.setenv("WB_CASC_WAVES", "8")
    assert [geometry(128, 2, shape, f)[:3] for f in ("f32", "rank16", "u8", "rank8")] == [(4, 8, 32), (4, 8, 32), (8, 8, 64), (8, 8, 64)]
    monkeypatch.setenv("WB_CASC_RPW", "4")
    assert {geometry(128, 2, shape, f)[:3] for f in FORMS} == {(4, 8, 32)}
    monkeypatch.setenv("WB_CASC_RPW", "2")
    assert {geometry(128, 2, shape, f)[:3] for f in FORMS} == {(2, 8, 16)}
    monkeypatch.delenv("WB_CASC_RPW")
    monkeypatch.setenv("WB_CASC_BYTE_RPW", "4")
    assert {geometry(128, 2, shape, f)[:3] for f in FORMS} == {(4, 8, 32)}
