"""tests/tools/gemm_blocks.py on the CPU: the numpy models of the two kernel families stay inside every bar of check_blocks over the
group-size ladder of tests/test_gpu_group_sizes.py, and two planted errors — a wrong scale row in one row block of one 16-column
tile, and in one row — pass the whole-output rel_l2 at 1e-3 and fail the block checks, which name the block.

Largest values the models showed here (rows 1 / 7 / 40 / 200 of one 200-row product per format, N = 263, K = 1920 / 2048 / 1952):
  tiled      (7 rows and more) against the fp32 oracle: row 3.8e-4, tile 3.9e-4, block 4.3e-4; against the fp16-activation oracle: row
             2.6e-4, tile 2.8e-4; term 5.6e-5
  streaming  against the fp32 oracle: row 3.6e-4, tile and block 8.2e-4 (one row: a tile is 16 numbers); term 5.2e-5; against the
             fp16-activation oracle 8e-7 on integer weights, row 2.5e-4 / tile 4.9e-4 on NF4 (the tiled model stands in)"""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("gemm_blocks", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gemm_blocks.py"))
gb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gb)

N = 263
KS = (1920, 2048, 1952)
LADDER = [  # qtype, scale dtype, asym, core, groups
    ("S4", "BF16", False, "CORE_AVX512_VNNI_KB", (128, 256, 384, 512, 640, -1)),
    ("S4", "F32", True, "CORE_AVX512F", (128, 256, 384, 512, 640, -1)),
    ("F4_NF4", "BF16", False, "CORE_AVX512F", (128, 256, 384, 512, 640, -1)),
    ("S4", "F16", False, "CORE_AVX512F", (384,)),
    ("S8", "BF16", False, "CORE_AVX512F", (64, 128, 192, 320, -1)),
    ("S8", "F32", True, "CORE_AVX512F", (64, 128, 192, 320, -1)),
    ("F8_E4M3", "F32", False, "CORE_AVX512F", (64, 128, 192, 320, -1)),
    ("F8_E4M3", "F8_E8M0", False, "CORE_AVX512F", (64, 128, 192, 320, -1)),
]
CASES = [(qt, st, asym, core, g, k) for qt, st, asym, core, groups in LADDER for g in groups for k in KS]


@pytest.mark.parametrize("qt,st,asym,core,group,k", CASES)
def test_models_stay_inside_every_bar(nso, qt, st, asym, core, group, k):
    """the model of a family, handed to check_blocks as if it were that family's kernel (its own model as the yardstick of the two
    measured bars, so those hold by construction; the fixed bars are what is checked)"""
    rng = np.random.default_rng(k * 7 + group + len(qt) + len(st))
    w = (rng.standard_normal((N, k)) * 0.02).astype(np.float32)
    a = rng.standard_normal((200, k)).astype(np.float32)
    blob = nso.quant_pack(w, group, getattr(nso, qt), getattr(nso, st), asym, getattr(nso, core))
    f4 = qt.startswith("F4")
    prob = gb.Problem(nso, a, blob, f4=f4)
    for family in ("stream", "tiled"):
        for m in (1, 7, 40, 200):
            if family == "tiled" and m == 1:
                continue  # one row never reaches a tiled kernel (they serve 17 rows and more), and the 5e-4 bar against the fp16-activation
                # oracle was set on their outputs: on the 16 numbers of a one-row tile the tiled model's weight rounding alone can pass it
            gb.check_blocks(nso, prob.model(family)[:m], a[:m], blob, family, prob=prob, what="%s model m=%d" % (family, m))


def _planted(nso, rows_bad, cols_bad):
    """a 257 x 263 product of S4 / BF16 weights in groups of 256 over K = 1952 (three-array layout: 8 scale rows, the last group 160
    deep, the last k-step 32 deep) in which the block rows_bad x cols_bad took the NEIGHBOURING scale row (6 instead of 7) for the
    last k-step.  The weights' largest magnitude alternates between 0.060 and 0.0612 from group to group, so the two scale rows differ
    by 2 % and the block is off by about 0.02 * sqrt(32 / 1952) = 2.6e-3 of its norm: diluted to 3e-4 in the whole output, under its
    1e-3 and 5e-4 bars"""
    rng = np.random.default_rng(11)
    m, k, g = 257, 1952, 256
    w = np.clip(rng.standard_normal((N, k)) * 0.02, -0.05, 0.05).astype(np.float32)
    for gi in range((k + g - 1) // g):
        w[:, gi * g] = 0.060 * (1.02 if gi % 2 else 1.0)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = nso.quant_pack(w, g, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    q, sc, _zp = nso.unpack_canonical(blob)
    wq = nso.unpack_fp32(blob)
    assert np.array_equal(wq, q.astype(np.float32) * np.repeat(sc, g, axis=0)[:k]), "the dequantised weight is code * scale row"
    s_last = (k - 1) // 128
    k0 = s_last * 128
    assert k0 // g == 7 and abs(float(np.median(sc[7] / sc[6])) - 1.02) < 5e-3
    wbad = wq.copy()
    wbad[k0:] = q[k0:].astype(np.float32) * sc[6]
    good = gb.model(a, wq, "tiled")
    out = good.copy()
    out[rows_bad, cols_bad] = gb.model(a, wbad, "tiled")[rows_bad, cols_bad]
    return out, good, a, blob


def test_one_wrong_tile_of_one_row_block_passes_the_tensor_metric_and_fails_the_block_check(nso):
    out, good, a, blob = _planted(nso, slice(64, 128), slice(5 * 16, 6 * 16))
    ref = nso.gemm_f64(a, blob)
    assert nso.rel_l2(good, ref) < gb.TOL and nso.rel_l2(out, ref) < gb.TOL, "the old metric does not see the planted block"
    gb.check_blocks(nso, good, a, blob, "tiled")
    with pytest.raises(gb.BlockCheckError) as info:
        gb.check_blocks(nso, out, a, blob, "tiled")
    named = {kind: (index, value) for _r, kind, index, value, _b in info.value.fails}
    assert named["block"][0] == (1, 5) and named["block"][1] > 2e-3, named
    # whatever else fails lies inside that block: its worst element, its tile, one of its rows — never the whole output
    assert set(named) <= {"block", "term", "tile f32", "tile a16", "row f32", "row a16"}, named
    for kind, (index, _v) in named.items():
        if kind == "term":
            assert 64 <= index[0] < 128 and 80 <= index[1] < 96, named
        elif kind.startswith("tile"):
            assert index == (5,), named
        elif kind.startswith("row"):
            assert 64 <= index[0] < 128, named


def test_one_wrong_row_passes_the_tensor_metric_and_fails_the_row_check(nso):
    out, good, a, blob = _planted(nso, slice(131, 132), slice(0, N))
    ref = nso.gemm_f64(a, blob)
    assert nso.rel_l2(out, ref) < gb.TOL, "the old metric does not see the planted row"
    with pytest.raises(gb.BlockCheckError) as info:
        gb.check_blocks(nso, out, a, blob, "tiled")
    kinds = {(kind, index) for _r, kind, index, _v, _b in info.value.fails}
    assert ("row f32", (131,)) in kinds, kinds
    assert info.value.index[0] in (131, 131 // 64), (info.value.kind, info.value.index)


def test_block_helpers_on_a_known_array():
    ref = np.ones((33, 40))
    out = ref.copy()
    out[32, 35] = 2.0
    assert gb.row_errors(out, ref).argmax() == 32 and gb.tile_errors(out, ref).shape == (3,)
    blk = gb.tile_row_block_errors(out, ref, 16)
    assert blk.shape == (3, 3) and blk[2, 2] == pytest.approx(1.0 / np.sqrt(8.0)) and np.count_nonzero(blk) == 1
    t = gb.term_errors(out, ref, np.ones((33, 4)), np.full((4, 40), 0.5))
    assert t.max() == pytest.approx(0.5) and np.count_nonzero(t) == 1
    # a last tile narrower than MIN_BLOCK joins its neighbour (17 columns: one tile); at 7 columns it stands alone
    assert gb.tile_errors(ref[:, :17], ref[:, :17]).shape == (1,) and gb.tile_errors(ref[:, :23], ref[:, :23]).shape == (2,)
    # ... and single-element rows are not held one by one: a 1-column output off by 1.5e-3 in one of 33 rows passes 1e-3 as a whole
    col = np.ones((33, 1))
    off = col.copy()
    off[5] += 1.5e-3
    gb.check_rows_tiles(off, col, 1e-3)
    with pytest.raises(gb.BlockCheckError):
        gb.check_rows_tiles(np.repeat(off, 7, axis=1), np.repeat(col, 7, axis=1), 1e-3)
