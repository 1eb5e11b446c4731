"""Block-wise checks of a quantised matrix product, as plain numpy: what tests/test_gemm_blocks.py (CPU) and the GPU suites of the
matrix kernels hold an output to beside the whole-output rel_l2.

A wrong scale row in one wave's share of a launch changes one row, or one 16-column tile of one row block, of the output; in the
rel_l2 of a 257 x 263 output such an error is diluted by sqrt(affected / total) and passes 1e-3.  So every output is compared
  * as a whole, row by row and 16-column tile by tile (over all rows) against the oracle's fp64 products of the fp32 activations
    (1e-3) and of the fp16-rounded activations (3e-5 integer / fp8 weights on the streaming kernels, 6e-4 f4 weights, 5e-4 the
    tiled kernels); in int8-reference mode against nso.gemm_u8s8 (2e-6 whole, 1e-5 per row and per tile).  None of these bars is
    new (tests/test_gpu_parity.py, tests/test_gpu_int8_mode.py); they are norm-wise relative, so what to expect of them does not
    depend on the size of the block;
  * per (16-column tile, block of `rows` rows) — 16 rows for the streaming kernels, whose waves own 16-row blocks, 64 for the tiled
    ones — and element by element as |out - ref| / (|a| @ |wq|) (term_errors: the yardstick of test_forward_weight_magnitudes,
    which cancellation in a sum cannot inflate), against a numpy MODEL of the kernel family computed on the same inputs:
        streaming   fp16-rounded activations x the exactly dequantised weights, fp32 accumulation
        tiled       the same with the dequantised weights rounded to fp16 as well
    (f4 weights on the streaming kernels round their 16-entry table to fp16: the tiled model stands in for them, the same 2^-12
    per weight).  The kernel is bounded by max(floor, factor x the model's error): per block for the block errors, worst against
    worst for the term errors.

The two measured bars (the rule of tests/test_gpu_attention_paths.py: ROW_FLOOR, ROW_FACTOR):
  BLOCK_FLOOR = 2^-12  the relative error of ONE operand rounded to fp16: a block is not asked to be closer than that
  TERM_FLOOR  = 2^-15  half of the largest term error the models themselves show (4.7e-5 streaming, 6.3e-5 tiled over the ladder of
                       tests/test_gemm_blocks.py): it decides only where the model's own error vanishes
  BLOCK_FACTOR, TERM_FACTOR: twice the largest ratio kernel / model that tests/test_gpu_group_sizes.py saw on the
  INTERLEAVED CONTROL formats (group 128 on 4-bit records, 64 on 8-bit and fp8 records — the layouts every other GPU test runs),
  never on the large-group formats they are then applied to; "ratio" is kernel / model over the blocks (for the terms: the worst
  element) whose kernel error is above the floor, which is what the factor has to cover.  Measured on an MI355X over every family
  of that module (gemv_kernel, gemvs_kernel, smallm_kernel; gemm2_kernel, gemm3_kernel, gemm_kernel for fp8, the grouped MoE path):
                 block ratio, control   factor   ladder saw     term ratio, control   factor   ladder saw
      streaming        1.84              3.7       2.21               1.14              2.3       1.38
      tiled            2.61              5.3       3.45               1.42              2.9       1.79
  (the block ratios are largest on the one-row last row block of a 257-row call: 16 numbers.)  Largest errors themselves, control
  / ladder: streaming block 6.6e-4 / 8.1e-4, term 4.3e-5 / 4.8e-5; tiled block 1.0e-3 / 7.4e-4, term 6.0e-5 / 8.6e-5; the fixed bars
  saw at most: rel_l2 3.6e-4 / 3.9e-4, row 4.2e-4 / 4.6e-4, tile 6.6e-4 / 6.7e-4 against the fp32 oracle (1e-3); tiled kernels
  against the fp16-activation oracle 3.5e-4 / 3.8e-4 (5e-4); int8-reference mode rel_l2 8.5e-7 / 9.2e-7 (2e-6), row, tile and block
  1.4e-6 / 1.9e-6 (1e-5).  docs/measurement.md ("Block-wise bars of the matrix kernels") has the same table.
A norm-wise bar needs a norm: the relative error of ONE element of a correct product has no bound (the sum it is compared with may
cancel), and the models themselves pass 1e-3 on single elements (a 1-column output, the 1-wide last tile of a 17-column one).  The
narrowest block the models were checked on is the 7-wide last tile of N = 263 at one row, so MIN_BLOCK = 7: a last tile narrower
than that is joined to its neighbour, and rows are held one by one only where the output has that many columns.

In int8-reference mode there is no model: the reference is fp32 arithmetic itself (another summation order), and a 16 x 16 block
has as many elements as a row of the 263-column outputs the per-row bar was set on, so the blocks are held to that bar (1e-5)."""
import numpy as np

TOL = 1e-3
TOL_A16_INT = 3e-5
TOL_A16_F4 = 6e-4
TOL_A16_GEMM = 5e-4
TOL_I8, TOL_I8_ROW = 2e-6, 1e-5
BLOCK_FLOOR = 2.0 ** -12
TERM_FLOOR = 2.0 ** -15
# family: (rows of a row block, BLOCK_FACTOR, TERM_FACTOR)
FACTORS = {"stream": (16, 3.7, 2.3), "tiled": (64, 5.3, 2.9)}
I8_BLOCK_ROWS = 16
TILE = 16
MIN_BLOCK = 7

# the largest value every bar saw, per (family, "control" / "ladder", kind): printed by the GPU modules, copied into docs/measurement.md
SEEN = {}


def _blocks(x, rows, cols):
    """sum of x over blocks of rows x cols -> [ceil(m / rows)][ceil(n / cols)]; a last column block of fewer than MIN_BLOCK columns
    belongs to the one before it"""
    m, n = x.shape
    starts = np.arange(0, n, cols)
    if len(starts) > 1 and n - starts[-1] < MIN_BLOCK:
        starts = starts[:-1]
    r = np.add.reduceat(x, np.arange(0, m, rows), axis=0)
    return np.add.reduceat(r, starts, axis=1)


def _rel(out, ref, rows, cols):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(_blocks((out - ref) ** 2, rows, cols) / np.maximum(_blocks(ref ** 2, rows, cols), 1e-300))


def rel_l2(out, ref):
    return float(_rel(out, ref, out.shape[0], out.shape[1])[0, 0])


def row_errors(out, ref):
    """rel_l2 of every row -> [m]"""
    return _rel(out, ref, 1, out.shape[1])[:, 0]


def tile_errors(out, ref):
    """rel_l2 of every 16-column tile over all rows -> [ceil(n / 16)] (one fewer where the last tile is narrower than MIN_BLOCK)"""
    return _rel(out, ref, out.shape[0], TILE)[0]


def tile_row_block_errors(out, ref, rows):
    """rel_l2 of every (block of `rows` rows, 16-column tile) -> [ceil(m / rows)][ceil(n / 16)]"""
    return _rel(out, ref, rows, TILE)


def term_errors(out, ref, a, wq):
    """|out - ref| / (|a| @ |wq|), element by element; wq: the dequantised weight, [K][N]"""
    mag = np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(wq, np.float64))
    return np.abs(np.asarray(out, np.float64) - np.asarray(ref, np.float64)) / np.maximum(mag, 1e-300)


def model(a, wq, family):
    """the numpy model of a kernel family (module docstring) on activations a [m][K] and the dequantised weight wq [K][N]"""
    a16 = np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
    w = np.asarray(wq, np.float32)
    if family == "tiled":
        w = w.astype(np.float16).astype(np.float32)
    return a16 @ w


class Problem:
    """the references of one (activations, blob): made once, shared by every call that multiplies the first m of these rows"""

    def __init__(self, nso, a, blob, f4=False, i8=False):
        self.a, self.f4 = np.ascontiguousarray(a, np.float32), f4
        self.wq = nso.unpack_fp32(blob)
        self.mag = np.abs(self.a.astype(np.float64)) @ np.abs(self.wq.astype(np.float64))
        self.ref, self.ref16 = nso.gemm_f64_pair(self.a, blob)
        self.ref8 = nso.gemm_u8s8(self.a, blob).astype(np.float64) if i8 else None
        self._model = {}

    def model(self, family):
        fam = "tiled" if self.f4 else family
        if fam not in self._model:
            self._model[fam] = model(self.a, self.wq, fam).astype(np.float64)
        return self._model[fam]

    @classmethod
    def of_rows(cls, probs, pick):
        """row t of the result is row t of probs[pick[t]] (one set of activations, an expert per row); None: a row of zeros"""
        p = cls.__new__(cls)
        first = next(q for q in probs if q is not None)
        p.a, p.f4, p.ref8 = first.a[:len(pick)], first.f4, None

        def rows(get):
            return np.stack([get(probs[e])[t] if e is not None else np.zeros(first.ref.shape[1]) for t, e in enumerate(pick)])
        p.ref, p.ref16, p.mag = rows(lambda q: q.ref), rows(lambda q: q.ref16), rows(lambda q: q.mag)
        p._model = {fam: rows(lambda q, fam=fam: q.model(fam)) for fam in ("stream", "tiled")}
        return p


def _note(family, control, kind, value):
    key = (family, "control" if control else "ladder", kind)
    SEEN[key] = max(SEEN.get(key, 0.0), float(value))


def _worst(fails, kind, err, bar):
    """records where `err` exceeds `bar` the most (as a ratio): (ratio, kind, index, value, bar)"""
    err, bar = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bar, np.float64), np.shape(err))
    ratio = err / bar
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
    if ratio[i] >= 1.0 or not np.isfinite(ratio[i]):
        fails.append((float(ratio[i]), kind, tuple(int(j) for j in i), float(err[i]), float(bar[i])))


class BlockCheckError(AssertionError):
    def __init__(self, what, fails):
        self.fails = sorted(fails, reverse=True)
        _r, self.kind, self.index, self.value, self.bar = self.fails[0]
        AssertionError.__init__(self, "%s: worst %s %s = %.3g (bar %.3g); all: %s" % (
            what, self.kind, self.index, self.value, self.bar, [(k, i, "%.3g" % v, "%.3g" % b) for _r, k, i, v, b in self.fails]))


def check_rows_tiles(out, ref, tol, what="", row_tol=None, tile_tol=None):
    """the epilogue form: whole output, every row and every 16-column tile of `out` within tol of `ref` (an fp64 epilogue of the
    oracle's product, say).  Returns (whole, worst row, worst tile)"""
    fails = []
    e, rows, tiles = rel_l2(out, ref), row_errors(out, ref), tile_errors(out, ref)
    _worst(fails, "rel_l2", np.float64(e), tol)
    if out.shape[1] >= MIN_BLOCK:
        _worst(fails, "row", rows, row_tol or tol)
    _worst(fails, "tile", tiles, tile_tol or row_tol or tol)
    if fails:
        raise BlockCheckError(what, fails)
    return e, float(rows.max()), float(tiles.max())


def check_blocks(nso, out, a, blob, family, prob=None, what="", control=False, f4=False, tol16=None):
    """`out` [m][n] (m rows of a kernel of `family`: "stream", "tiled" or "i8") against the references of (a, blob): every bar of
    the module docstring.  prob: a Problem of (a', blob) with a = a'[:m], to share its references; tol16: the fp16-activation bar of a
    kernel that has one of its own.  Raises BlockCheckError naming
    the worst (kind, index, value); returns {kind: largest value seen}"""
    out = np.asarray(out)
    m = out.shape[0]
    if prob is None:
        prob = Problem(nso, a, blob, f4=f4, i8=family == "i8")
    fails, seen = [], {}

    def hold(kind, err, bar):
        seen[kind] = float(np.max(err))
        _note(family, control, kind, seen[kind])
        _worst(fails, kind, err, bar)

    if family == "i8":
        ref = prob.ref8[:m]
        hold("rel_l2 u8s8", np.float64(rel_l2(out, ref)), TOL_I8)
        if out.shape[1] >= MIN_BLOCK:
            hold("row u8s8", row_errors(out, ref), TOL_I8_ROW)
        hold("tile u8s8", tile_errors(out, ref), TOL_I8_ROW)
        hold("block u8s8", tile_row_block_errors(out, ref, I8_BLOCK_ROWS), TOL_I8_ROW)
    else:
        rows, bfac, tfac = FACTORS[family]
        ref, ref16, mod = prob.ref[:m], prob.ref16[:m], prob.model(family)[:m]
        tol16 = tol16 or (TOL_A16_F4 if prob.f4 else (TOL_A16_GEMM if family == "tiled" else TOL_A16_INT))
        for name, r, tol in (("f32", ref, TOL), ("a16", ref16, tol16)):
            hold("rel_l2 " + name, np.float64(rel_l2(out, r)), tol)
            if out.shape[1] >= MIN_BLOCK:
                hold("row " + name, row_errors(out, r), tol)
            hold("tile " + name, tile_errors(out, r), tol)
        blk, blk_m = tile_row_block_errors(out, ref, rows), tile_row_block_errors(mod, ref, rows)
        bar = np.maximum(BLOCK_FLOOR, bfac * blk_m)
        hold("block", blk, bar)
        over = blk > BLOCK_FLOOR   # the blocks the factor decides: what it has to be at least
        _note(family, control, "block / model above the floor", np.max(blk[over] / np.maximum(blk_m[over], 1e-300)) if over.any() else 0.0)
        mag = prob.mag[:m]
        term = np.abs(out.astype(np.float64) - ref) / np.maximum(mag, 1e-300)
        term_m = float(np.max(np.abs(mod - ref) / np.maximum(mag, 1e-300)))
        hold("term", term, max(TERM_FLOOR, tfac * term_m))
        _note(family, control, "term / model above the floor", term.max() / max(term_m, 1e-300) if term.max() > TERM_FLOOR else 0.0)
    if fails:
        raise BlockCheckError(what, fails)
    return seen


def seen_report():
    return {" ".join(k): "%.3g" % v for k, v in sorted(SEEN.items())}
