"""Channel quantizers and adversarial LLRs shared by tests/test_llr_input.py (CPU)
and tests/test_gpu_llr_input.py: every edge, nextafter on both sides of it, +-inf,
+-0, the float32 values around each edge, and random LLRs over the edges' range."""
import numpy as np


def quantizers(lutgen=None):
    """{name: (edges, lut, q)}.  ``lutgen``: the module, for the drivers' MinDistortion
    design (needs libqpd.so's host code); left out without it."""
    from quantized_decoder_polar_codes_amd import montecarlo as MC

    out = {}
    e, l = MC.uniform_channel_quantizer(16, 0.5)
    out["uniform"] = (e, l, 16)
    if lutgen is not None:
        _, _, e, l = lutgen.channel_quantizer(0.8, 128, 16)
        out["mindistortion"] = (np.asarray(e, dtype=np.float64), np.asarray(l, dtype=np.int32), 16)
    out["edges2"] = (np.array([-0.25, 1.5]), np.array([1], dtype=np.int32), 3)
    rng = np.random.default_rng(257)
    e = np.sort(rng.normal(0, 6, size=257))
    out["edges257"] = (e, rng.integers(0, 16, size=256).astype(np.int32), 16)
    # duplicates inside and at both ends; an edge at -0.0 and one that is a float32
    e = np.array([-3.0, -3.0, -1.5, -0.0, 0.0, 0.0, 0.75, 0.75, 0.75, 2.0, 4.0, 4.0])
    out["duplicates"] = (e, np.array([3, 0, 1, 5, 2, 4, 4, 6, 7, 1, 0], dtype=np.int32), 8)
    return out


def adversarial(edges, n_random=0, seed=0):
    """float64 LLRs: the cases above, then n_random normal draws over the edges' range."""
    e = np.asarray(edges, dtype=np.float64)
    f = e.astype(np.float32)
    # the specials first: a short prefix of the result still saturates both ways
    parts = [np.array([-np.inf, np.inf, 0.0, -0.0, 1e300, -1e300, 5e-324, -5e-324]),
             e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
             f.astype(np.float64), np.nextafter(f, np.float32(-np.inf)).astype(np.float64),
             np.nextafter(f, np.float32(np.inf)).astype(np.float64)]
    if n_random:
        span = max(1.0, float(e[-1] - e[0]))
        parts.append(np.random.default_rng(seed).normal((e[0] + e[-1]) / 2, span, size=n_random))
    return np.concatenate(parts)


def frames(x, N, B, dtype=np.float64):
    """x (float64) tiled / cut to [B, N] of dtype; float32 keeps what the cast leaves
    (the kernel widens it back exactly)."""
    reps = -(-B * N // x.size)
    with np.errstate(over="ignore"):  # 1e300 as float32 is inf, on purpose
        return np.ascontiguousarray(np.tile(x, reps)[: B * N].reshape(B, N).astype(dtype))
