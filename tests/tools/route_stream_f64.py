"""An fp64 numpy model of the token stream tests/test_gpu_route_replay.py::_run_layers issues on the device route, and the inputs the route-edge
tests run it on.  Per token, NL decoder layers sharing one set of weights and one norm weight:
    h = rms_norm(x) . gamma;  K, V, Q = h Wk, h Wv, h Wq;  RoPE (mode 0: adjacent pairs, all HS dims) on K and Q at the token's position;
    K, V into the caches at that position;  attention of every query head over position 0 .. pos of its kv head, scale HS ** -0.5;
    r = x + attn Wo;  h2 = rms_norm(r) . gamma;  x' = r + (silu(h2 W1) * (h2 W3)) W2
then the last norm and the projection by W1.  Weights are the oracle's dequantisation of the packed blobs (nso.unpack_fp32, [k][n]) in fp64, every sum
is an fp64 sum.  a16=True rounds the activations of every projection to fp16 first (what nso.gemm_f64(..., a16=True) does to its left operand): the
difference between the two runs says how much of an error against this model is the inputs' conditioning and not the kernels'.
numpy only; nothing here touches the GPU."""
import numpy as np

D, FF, HEADS, HS, NCTX, NL = 512, 1408, 4, 128, 64, 2
EPS, ROPE_BASE = 1e-5, 10000.0
F16_MAX = 65504.0
WEIGHTS = ("wq", "wk", "wv", "wo", "w1", "w3", "w2")


def unpack(nso, blobs):
    return {name: nso.unpack_fp32(blobs[name]).astype(np.float64) for name in WEIGHTS}


def _rms(x, gam):
    return x / np.sqrt((x * x).mean() + EPS) * gam


def _rope(x, pos):  # x [heads][HS]
    th = pos * (ROPE_BASE ** (-2.0 / HS)) ** np.arange(HS // 2)
    c, s = np.cos(th), np.sin(th)
    out = x.copy()
    out[:, 0::2] = x[:, 0::2] * c - x[:, 1::2] * s
    out[:, 1::2] = x[:, 0::2] * s + x[:, 1::2] * c
    return out


def run(W, gam, xs, nctx=NCTX, pos0=0, cache0=None, hkv=HEADS, poke=None, a16=False, nl=NL):
    """W: unpack(...); gam, xs as _run_layers takes them; nl: layers; cache0: nl K caches [hkv][nctx][HS] then nl V caches [hkv][HS][nctx], flat; poke: (token, position,
    rows[layer][kv head]) — K rows written into the caches in front of that token.  Returns a dict:
      outs[t]                      the token's FF outputs
      caches                       as _run_layers returns them (K caches, then V caches, flat)
      max_k, max_v, max_gr, max_score   [t][layer]: the largest |K| and |V| the token writes, the largest |gamma . residual| (both residual adds of the layer:
                                   what a carried norm's fp16 shadow holds), the largest |score| of its attention"""
    gam = np.asarray(gam, np.float64)
    act = (lambda a: a.astype(np.float16).astype(np.float64)) if a16 else (lambda a: a)
    Kc = [np.zeros((hkv, nctx, HS)) if cache0 is None else np.asarray(cache0[il], np.float64).reshape(hkv, nctx, HS).copy() for il in range(nl)]
    Vc = [np.zeros((hkv, HS, nctx)) if cache0 is None else np.asarray(cache0[nl + il], np.float64).reshape(hkv, HS, nctx).copy() for il in range(nl)]
    group = HEADS // hkv
    res = {"outs": [], "max_k": [], "max_v": [], "max_gr": [], "max_score": []}
    for tok, x in enumerate(xs):
        pos = pos0 + tok
        if poke is not None and tok == poke[0]:
            for il in range(nl):
                for h_ in range(hkv):
                    Kc[il][h_, poke[1]] = np.asarray(poke[2][il][h_], np.float64)
        x = np.asarray(x, np.float64)
        mk, mv, mgr, ms = [], [], [], []
        for il in range(nl):
            h = act(_rms(x, gam))
            k = _rope((h @ W["wk"]).reshape(hkv, HS), pos)
            v = (h @ W["wv"]).reshape(hkv, HS)
            q = _rope((h @ W["wq"]).reshape(HEADS, HS), pos)
            Kc[il][:, pos] = k
            Vc[il][:, :, pos] = v
            o = np.zeros((HEADS, HS))
            smax = 0.0
            for hq in range(HEADS):
                hk = hq // group
                s = Kc[il][hk, :pos + 1] @ q[hq] * HS ** -0.5
                smax = max(smax, float(np.abs(s).max()))
                p = np.exp(s - s.max())
                o[hq] = Vc[il][hk, :, :pos + 1] @ (p / p.sum())
            r = x + act(o.reshape(-1)) @ W["wo"]
            h2 = act(_rms(r, gam))
            gate, up = h2 @ W["w1"], h2 @ W["w3"]
            x = r + act(gate / (1.0 + np.exp(-gate)) * up) @ W["w2"]
            mk.append(float(np.abs(k).max())), mv.append(float(np.abs(v).max())), ms.append(smax)
            mgr.append(float(max(np.abs(gam * r).max(), np.abs(gam * x).max())))
        res["outs"].append(act(_rms(x, gam)) @ W["w1"])
        res["max_k"].append(mk), res["max_v"].append(mv), res["max_gr"].append(mgr), res["max_score"].append(ms)
    res["caches"] = [c.reshape(-1) for c in Kc + Vc]
    return res


def _pack(nso, w):
    return nso.quant_pack(np.ascontiguousarray(w, np.float32), 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)


def ordinary_inputs(nso, seed, ntok):
    """the inputs the existing route cases use: weights N(0, 1 / k), gamma 1 +- 0.1, tokens N(0, 1)"""
    rng = np.random.default_rng(seed)
    mk = lambda n, k: _pack(nso, rng.standard_normal((n, k)) * k ** -0.5)
    blobs = {"wq": mk(D, D), "wk": mk(D, D), "wv": mk(D, D), "wo": mk(D, D), "w1": mk(FF, D), "w3": mk(FF, D), "w2": mk(D, FF)}
    gam = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    xs = [rng.standard_normal(D).astype(np.float32) for _ in range(ntok)]
    return blobs, gam, xs


def first_token_overflow_inputs(nso, ntok=8):
    """the inputs of test_values_beyond_fp16_turn_the_fp16_shortcuts_off_and_the_token_is_evaluated_again (seed 8): the whole key projection scaled by 1e5,
    the query projection by 1e-4 — K leaves the fp16 range at the first token"""
    rng = np.random.default_rng(8)
    mk = lambda n, k, s=1.0: _pack(nso, rng.standard_normal((n, k)) * s * k ** -0.5)
    blobs = {"wq": mk(D, D, 1e-4), "wk": mk(D, D, 1e5), "wv": mk(D, D), "wo": mk(D, D), "w1": mk(FF, D), "w3": mk(FF, D), "w2": mk(D, FF)}
    gam = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    xs = [rng.standard_normal(D).astype(np.float32) for _ in range(ntok)]
    return blobs, gam, xs


T_OV, J0, OV_SEED = 5, 77, 41
OV_C, OV_WQ_SCALE = 8e3, 3e-5  # (c = 1.5e4 with the query scale 1e-4 of the existing overflow case: scores up to 62, fp16-activation sensitivity 7e-4; these: 10 and 4e-4)


def overflow_inputs(nso, ntok=10, t_ov=T_OV, seed=OV_SEED, c=OV_C, wq_scale=OV_WQ_SCALE):
    """Inputs whose K leaves the fp16 range at token t_ov and at no other.  rms_norm removes a token's scale, so the token's DIRECTION does it: column J0 of the
    key projection (the weights that multiply feature J0) is +-c . U(0.5, 1); every token has x[J0] = 0 except token t_ov = 100 e_J0 + N(0, 1), whose normed
    feature J0 is ~ sqrt(D) gamma[J0].  Row J0 of wo and of w2 (the weights that produce feature J0) is zero, so the residual's feature J0 stays exactly
    what the token brought in EVERY layer (the layers share their weights): exactly 0 for the ordinary tokens — K is moderate in both layers — and 100 at
    t_ov.  The query projection is scaled down so that the scores against the large key stay moderate."""
    rng = np.random.default_rng(seed)
    raw = lambda n, k, s=1.0: rng.standard_normal((n, k)) * s * k ** -0.5
    wq, wk, wv, wo, w1, w3, w2 = raw(D, D, wq_scale), raw(D, D), raw(D, D), raw(D, D), raw(FF, D), raw(FF, D), raw(D, FF)
    wk[:, J0] = c * rng.uniform(0.5, 1.0, D) * rng.choice([-1.0, 1.0], D)
    wo[J0, :] = 0.0
    w2[J0, :] = 0.0
    blobs = {"wq": _pack(nso, wq), "wk": _pack(nso, wk), "wv": _pack(nso, wv), "wo": _pack(nso, wo), "w1": _pack(nso, w1), "w3": _pack(nso, w3),
             "w2": _pack(nso, w2)}
    gam = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    xs = [rng.standard_normal(D).astype(np.float32) for _ in range(ntok)]
    for x in xs:
        x[J0] = 0.0
    xs[t_ov][J0] = 100.0
    return blobs, gam, xs


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
