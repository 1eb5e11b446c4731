"""tests/tools/route_stream_f64.py — the fp64 model the route-edge GPU cases (test_gpu_route_edges.py) take their expected values from — checked on the
CPU against what can be written out by hand, and the conditions the overflow inputs must satisfy for the exact seeds the GPU cases use."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import route_stream_f64 as rs  # noqa: E402

F16_MAX = 65504.0


def test_one_layer_one_token_empty_cache_equals_the_closed_form(nso):
    """Attention over ONE key returns that key's V whatever the score is, and RoPE at position 0 is the identity: one layer over an empty cache is
    out = rms(x') g W1, x' = r + (silu(h2 W1) * (h2 W3)) W2, h2 = rms(r) g, r = x + (rms(x) g Wv) Wo; the cache rows are rms(x) g Wk and rms(x) g Wv."""
    blobs, gam, xs = rs.ordinary_inputs(nso, 5, 1)
    W = rs.unpack(nso, blobs)
    m = rs.run(W, gam, xs, nl=1)
    x, g = xs[0].astype(np.float64), gam.astype(np.float64)
    rms = lambda a: a / np.sqrt(np.mean(a * a) + 1e-5) * g
    h = rms(x)
    r = x + (h @ W["wv"]) @ W["wo"]
    h2 = rms(r)
    gate = h2 @ W["w1"]
    x1 = r + (gate / (1.0 + np.exp(-gate)) * (h2 @ W["w3"])) @ W["w2"]
    want = rms(x1) @ W["w1"]
    assert m["outs"][0].shape == (rs.FF,) and np.allclose(m["outs"][0], want, rtol=1e-12, atol=1e-12)
    kc, vc = m["caches"][0].reshape(rs.HEADS, rs.NCTX, rs.HS), m["caches"][1].reshape(rs.HEADS, rs.HS, rs.NCTX)
    assert np.allclose(kc[:, 0], (h @ W["wk"]).reshape(rs.HEADS, rs.HS), rtol=1e-12, atol=1e-12)
    assert np.allclose(vc[:, :, 0], (h @ W["wv"]).reshape(rs.HEADS, rs.HS), rtol=1e-12, atol=1e-12)
    assert not kc[:, 1:].any() and not vc[:, :, 1:].any()
    assert m["max_k"][0][0] == np.abs(kc).max() and m["max_v"][0][0] == np.abs(vc).max()


def test_rope_and_attention_of_the_model_at_a_later_position(nso):
    """Second token of a one-layer stream, by hand: K rotated by pos . theta_i in adjacent pairs, softmax over the two scores, V mixed by it."""
    blobs, gam, xs = rs.ordinary_inputs(nso, 5, 2)
    W = rs.unpack(nso, blobs)
    m = rs.run(W, gam, xs, nl=1, pos0=3)
    g = gam.astype(np.float64)
    rms = lambda a: a / np.sqrt(np.mean(a * a) + 1e-5) * g

    def rot(v, pos):
        v = v.reshape(rs.HEADS, rs.HS // 2, 2)
        th = pos * 10000.0 ** (-2.0 * np.arange(rs.HS // 2) / rs.HS)
        return np.stack([v[..., 0] * np.cos(th) - v[..., 1] * np.sin(th), v[..., 0] * np.sin(th) + v[..., 1] * np.cos(th)], -1).reshape(rs.HEADS, rs.HS)
    h0, h1 = rms(xs[0].astype(np.float64)), rms(xs[1].astype(np.float64))
    k0, k1, q1 = rot(h0 @ W["wk"], 3), rot(h1 @ W["wk"], 4), rot(h1 @ W["wq"], 4)
    v0, v1 = (h0 @ W["wv"]).reshape(rs.HEADS, rs.HS), (h1 @ W["wv"]).reshape(rs.HEADS, rs.HS)
    # positions 0 .. 2 of the cache are zero keys (score 0) with zero values: they take their share of the softmax
    o = np.zeros((rs.HEADS, rs.HS))
    for hh in range(rs.HEADS):
        s = np.array([0.0, 0.0, 0.0, k0[hh] @ q1[hh], k1[hh] @ q1[hh]]) * rs.HS ** -0.5
        p = np.exp(s) / np.exp(s).sum()
        o[hh] = p[3] * v0[hh] + p[4] * v1[hh]
    x = xs[1].astype(np.float64)
    r = x + o.reshape(-1) @ W["wo"]
    h2 = rms(r)
    gate = h2 @ W["w1"]
    x1 = r + (gate / (1.0 + np.exp(-gate)) * (h2 @ W["w3"])) @ W["w2"]
    assert np.allclose(m["outs"][1], rms(x1) @ W["w1"], rtol=1e-10, atol=1e-10)
    assert np.allclose(m["caches"][0].reshape(rs.HEADS, rs.NCTX, rs.HS)[:, 4], k1, rtol=1e-12, atol=1e-12)


def test_the_models_fp16_activation_rounding_is_the_oracles(nso):
    """a16=True rounds a projection's activations as nso.gemm_f64(..., a16=True) does"""
    blobs, gam, xs = rs.ordinary_inputs(nso, 5, 1)
    W = rs.unpack(nso, blobs)
    a = xs[0][None, :]
    assert np.allclose(a.astype(np.float16).astype(np.float64) @ W["wk"], nso.gemm_f64(a, blobs["wk"], a16=True), rtol=1e-12, atol=1e-12)
    assert np.allclose(a.astype(np.float64) @ W["wk"], nso.gemm_f64(a, blobs["wk"]), rtol=1e-12, atol=1e-12)


def test_a_poke_and_initial_caches_are_honoured(nso):
    blobs, gam, xs = rs.ordinary_inputs(nso, 10, 4)
    W = rs.unpack(nso, blobs)
    rng = np.random.default_rng(1)
    cache0 = [rng.standard_normal(rs.HEADS * rs.NCTX * rs.HS).astype(np.float32) for _ in range(2 * rs.NL)]
    plain = rs.run(W, gam, xs, pos0=8, cache0=cache0)
    assert np.array_equal(plain["caches"][0].reshape(rs.HEADS, rs.NCTX, rs.HS)[:, :8], cache0[0].reshape(rs.HEADS, rs.NCTX, rs.HS)[:, :8].astype(np.float64))
    rows = [[(3.0 * rng.standard_normal(rs.HS)).astype(np.float32) for _ in range(rs.HEADS)] for _ in range(rs.NL)]
    poked = rs.run(W, gam, xs, pos0=8, cache0=cache0, poke=(2, 1, rows))
    assert all(np.array_equal(a, b) for a, b in zip(plain["outs"][:2], poked["outs"][:2]))
    assert rs.rel_l2(poked["outs"][2], plain["outs"][2]) > 1e-3
    assert np.array_equal(poked["caches"][1].reshape(rs.HEADS, rs.NCTX, rs.HS)[2, 1], rows[1][2].astype(np.float64))


@pytest.mark.parametrize("t_ov", [rs.T_OV, 3])
def test_overflow_inputs_leave_the_fp16_range_at_the_chosen_token_only_and_are_well_conditioned(nso, t_ov):
    """The conditions of the inputs test_gpu_route_edges.py overflows a REPLAYED token with (seed, c and the query scale as committed):
      * before T_OV, every layer: max|K|, max|V|, max|gamma . residual| <= 65504 / 4 (no fp16 shortcut is near its range);
      * at T_OV: some |K| >= 2 x 65504 (no rounding decides whether the flag rises);
      * rounding every projection's activations to fp16 moves no token's output by more than 1e-3 rel-l2, T_OV and later included (what the GPU kernels may
        differ by from the fp64 model is then rounding, not conditioning).
    T_OV is a token the plan replays: tokens 0, 1 make the plan, 2 .. T_OV - 1 are replayed before it (5, and 3: see test_gpu_route_edges.py)."""
    assert rs.T_OV == 5 and t_ov >= 3
    blobs, gam, xs = rs.overflow_inputs(nso, t_ov=t_ov)
    assert len(xs) > t_ov + 2
    W = rs.unpack(nso, blobs)
    assert not W["wo"][:, rs.J0].any() and not W["w2"][:, rs.J0].any()   # (nothing writes feature J0 of the residual)
    m, m16 = rs.run(W, gam, xs), rs.run(W, gam, xs, a16=True)
    for t in range(t_ov):
        for il in range(rs.NL):
            assert max(m["max_k"][t][il], m["max_v"][t][il], m["max_gr"][t][il]) <= F16_MAX / 4, (t, il, m["max_k"][t][il], m["max_v"][t][il], m["max_gr"][t][il])
    assert m["max_k"][t_ov][0] >= 2 * F16_MAX, m["max_k"][t_ov]
    for t in range(t_ov + 1, len(xs)):   # (the tokens behind it write moderate rows again: ONE message on stderr is the whole story)
        assert max(max(m["max_k"][t]), max(m["max_v"][t])) <= F16_MAX / 4
    worst = max(rs.rel_l2(a, b) for a, b in zip(m16["outs"], m["outs"]))
    print("overflow inputs: max|K| at T_OV %.4g, largest |score| %.3g, fp16-activation sensitivity %.3g" %
          (max(m["max_k"][t_ov]), max(max(r) for r in m["max_score"]), worst))
    assert worst <= 1e-3, [rs.rel_l2(a, b) for a, b in zip(m16["outs"], m["outs"])]
    assert all(np.all(np.isfinite(o)) for o in m["outs"])


def test_first_token_overflow_inputs_are_the_existing_cases_and_well_conditioned(nso):
    """the inputs of the existing overflow case (seed 8): K beyond fp16 from the first token on, and the same conditioning bound"""
    blobs, gam, xs = rs.first_token_overflow_inputs(nso)
    W = rs.unpack(nso, blobs)
    m, m16 = rs.run(W, gam, xs), rs.run(W, gam, xs, a16=True)
    assert m["max_k"][0][0] >= 2 * F16_MAX
    worst = max(rs.rel_l2(a, b) for a, b in zip(m16["outs"], m["outs"]))
    print("first-token overflow inputs: max|K| %.4g, largest |score| %.3g, fp16-activation sensitivity %.3g" %
          (m["max_k"][0][0], max(max(r) for r in m["max_score"]), worst))
    assert worst <= 1e-3
