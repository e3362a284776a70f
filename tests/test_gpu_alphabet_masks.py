"""GPU parity away from the one point of the input space every other decode test uses (v = 16 and the frozen
mask of a nested reliability order): alphabets of 2 .. 256 symbols and the random, block-structured and edge
masks of tests/code_masks.py, against the CPU oracle (pinned to the reference there by
test_oracle_alphabet_masks.py).

What the kernels do with these inputs and with no other: the fast engine indexes quanta rows [j * v + sym],
loads a quanta row into 16 lanes behind `s16 < v` guards, keeps [temp][v] rank words for R1 nodes and tests
`s >= v` on nibble-packed channel symbols (at v = 8 a symbol 8 .. 15 fits the nibble: only that test catches
it); the mask drives the frozen-prefix stages, the register-resident bottom subtrees, the folded special nodes
and the three R1 argsort paths (<= 16, 17 .. 32, > 32 elements).  Every case asserts the engine that ran."""
import numpy as np
import pytest

import code_masks as M
from conftest import assert_engine, assert_frames_equal

pytestmark = pytest.mark.gpu

KINDS = ["SC-LUT", "SCL-LUT", "FastSC-LUT", "FastSCL-LUT"]
ENGINES = ["auto", "generic"]
ENV = ("QPD_NO_PFX", "QPD_NO_PRE", "QPD_NO_BFUSE", "QPD_LDS_BUDGET", "QPD_SETS", "QPD_PFX1B", "QPD_PRE_CHUNK")
FAST, GENERIC = 2, 1  # qpd_info.engine


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def _set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _pw(N, K):
    from quantized_decoder_polar_codes_amd import codes as C

    _, mb, fm, _ = C.construct_pw(N, K)
    return fm, C.identify_nodes(N, mb).astype(np.int32)


def _tables(N, v, tables, seed):
    from quantized_decoder_polar_codes_amd import lut as LU

    if tables == "minsum":
        return LU.minsum_uniform_luts(N, v=v)
    return LU.random_luts(N, v, seed=seed, distinct_mags=3, node_rows=(tables == "noderows"),
                          per_element=(tables == "perelem"))


def _symbols(N, v, B, seed):
    return np.random.default_rng(seed).integers(0, v, size=(B, N), dtype=np.int32)


def _served_fast(kind, L):
    """engine="auto" at v <= 16 and one table per node: the fast engine up to L = 8, SCL-LUT up to 16."""
    return "SCL" not in kind or L <= 8 or (L <= 16 and kind == "SCL-LUT")


def _parity(qpd, oracle_mod, kind, p, fm, nt, L, sym, engine, ran, label):
    """One decode against the oracle on `engine`; the decoder must report the engine `ran`."""
    K = int((np.asarray(fm) == 0).sum())
    want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
    dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine)
    assert dec.info()["engine"] == ran, (label, dec.info()["engine"])
    got = dec.decode_batch(sym)
    redo = lambda rows: qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine).decode_batch(sym[rows])  # noqa: E731
    assert_frames_equal(got, want, dec, label, redo, sym)
    return dec


def _refused_on_both_sides(qpd, oracle_mod, kind, p, fm, nt, L, sym, engine):
    K = int((np.asarray(fm) == 0).sum())
    with pytest.raises(RuntimeError):
        oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
    with pytest.raises(ValueError):
        qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine)


# ---------------------------------------------------------------------------------------------------------
# alphabets on the fast engine
# ---------------------------------------------------------------------------------------------------------

FAST_V = [2, 3, 8, 15]
PW_SHAPES = [(16, 8, 4), (128, 48, 8), (256, 128, 8)]
FAST_TABLES = [(v, t) for v in FAST_V for t in ("ties", "noderows")] + [(8, "minsum")]


@pytest.mark.parametrize("N,K,L", PW_SHAPES)
@pytest.mark.parametrize("v,tables", FAST_TABLES)
@pytest.mark.parametrize("kind", KINDS)
def test_fast_engine_alphabet(kind, v, tables, N, K, L, qpd, oracle_mod, monkeypatch):
    """Tie-heavy tables with per-element quanta ("ties") and with one quanta row per node ("noderows": the
    uniform-row and rank-word paths), at v = 8 also the min-sum tables."""
    _set_env(monkeypatch, {})
    fm, nt = _pw(N, K)
    assert not M.special_root(fm, kind)
    p = _tables(N, v, tables, seed=40 * N + v)
    sym = _symbols(N, v, 96, N + v + L)
    _parity(qpd, oracle_mod, kind, p, fm, nt, L, sym, "auto", FAST, f"alpha-{kind}-v{v}-{tables}-{N}-{K}-{L}")


@pytest.mark.parametrize("v,tables", FAST_TABLES)
def test_fast_engine_alphabet_every_prefix_stage(v, tables, qpd, oracle_mod, monkeypatch):
    """(128, 48, 8) with stage 1b asked for: ops in all three frozen-prefix stages (test_gpu_prefix.py)."""
    N, K, L = 128, 48, 8
    fm, nt = _pw(N, K)
    p = _tables(N, v, tables, seed=40 * N + v)
    sym = _symbols(N, v, 96, N + v + L)
    _set_env(monkeypatch, {})
    plain = qpd.from_packed("SCL-LUT", p, K, fm, L=L, engine="auto").info()["prefix_ops"]
    _set_env(monkeypatch, {"QPD_PFX1B": "1"})
    dec = _parity(qpd, oracle_mod, "SCL-LUT", p, fm, nt, L, sym, "auto", FAST, f"alpha-pfx1b-v{v}-{tables}")
    assert dec.info()["prefix_ops"] > plain > 0  # stage 1b taken


@pytest.mark.parametrize("v,tables", FAST_TABLES)
@pytest.mark.parametrize("kind,engine", [("SCL-LUT", "auto"), ("FastSCL-LUT", "fast")])
def test_fast_engine_alphabet_l16(kind, engine, v, tables, qpd, oracle_mod, monkeypatch):
    """L = 16: lane groups of 16 (select_survivors16); FastSCL-LUT gets them on request only."""
    _set_env(monkeypatch, {})
    N, K, L = 128, 64, 16
    fm, nt = _pw(N, K)
    p = _tables(N, v, tables, seed=40 * N + v + 1)
    sym = _symbols(N, v, 96, N + v + L)
    _parity(qpd, oracle_mod, kind, p, fm, nt, L, sym, engine, FAST, f"alpha-l16-{kind}-v{v}-{tables}")


# ---------------------------------------------------------------------------------------------------------
# alphabets on the generic engine
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tables", ["ties", "noderows"])
@pytest.mark.parametrize("v", [17, 32, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_generic_engine_alphabet(kind, v, tables, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    N = 32 if v == 256 else 128
    K, L = N // 2, 8
    fm, nt = _pw(N, K)
    assert not M.special_root(fm, kind)
    p = _tables(N, v, tables, seed=50 * N + v)
    sym = _symbols(N, v, 96, N + v)
    sym[0, :2] = (0, v - 1)  # both ends of the alphabet
    _parity(qpd, oracle_mod, kind, p, fm, nt, L, sym, "auto", GENERIC, f"alpha-generic-{kind}-v{v}-{tables}")


def test_fast_engine_refuses_v17(qpd):
    N, K = 32, 16
    fm, nt = _pw(N, K)
    with pytest.raises(ValueError):
        qpd.from_packed("SCL-LUT", _tables(N, 17, "ties", 1), K, fm, L=4, engine="fast")


@pytest.mark.parametrize("kind", KINDS)
def test_generic_engine_per_element_tables_v8(kind, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    N, K, L, v = 64, 32, 8, 8
    fm, nt = _pw(N, K)
    assert not M.special_root(fm, kind)
    p = _tables(N, v, "perelem", seed=77)
    _parity(qpd, oracle_mod, kind, p, fm, nt, L, _symbols(N, v, 96, 78), "auto", GENERIC, f"alpha-perelem-{kind}-v8")


# ---------------------------------------------------------------------------------------------------------
# the symbol v itself
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["host_buffer", "torch_device"])
@pytest.mark.parametrize("engine,ran", [("auto", FAST), ("generic", GENERIC)])
@pytest.mark.parametrize("kind", ["SCL-LUT", "FastSC-LUT"])
@pytest.mark.parametrize("v", [3, 8])
def test_symbol_v_is_out_of_range(v, kind, engine, ran, path, qpd, oracle_mod, monkeypatch):
    """A frame holding the symbol v -- which fits the nibble the fast kernels pack symbols in -- is reported,
    in the root's first half and in its second (the pre-pass reads the channel too), through the host-buffer
    call and through the device call; the next good batch decodes to the oracle's bits."""
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    _set_env(monkeypatch, {})
    N, K, L = 128, 64, 4
    fm, nt = _pw(N, K)
    p = _tables(N, v, "noderows", seed=60 + v)
    sym = _symbols(N, v, 40, 61 + v)
    want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
    dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine)
    assert dec.info()["engine"] == ran

    def decode(x):
        if path == "host_buffer":
            return dec.decode_batch(x)
        out = dec.decode_batch(torch.from_numpy(x).cuda())
        _lib.check(_lib.load().qpd_check_input_error(dec._h))  # waits for the launch; raises on a flagged symbol
        return out.cpu().numpy()

    for pos in (5, N // 2 + 5):
        bad = sym.copy()
        bad[17, pos] = v
        with pytest.raises(ValueError, match="outside"):
            decode(bad)
        assert_engine(dec, "gpu")
        assert_frames_equal(decode(sym), want, dec, f"symbol-v-{kind}-v{v}-{engine}-{path}-{pos}", None, sym)


# ---------------------------------------------------------------------------------------------------------
# masks, on both engines
# ---------------------------------------------------------------------------------------------------------

MASKS = ([(N, f"block{s}") for N in (64, 256) for s in M.BLOCK_SEEDS[N]]
         + [(N, name) for N in (16, 256) for name in M.EDGE_NAMES])


def _mask_case(qpd, oracle_mod, kind, v, engine, fm, L, B, label, ran=None, tables="noderows"):
    fm = np.asarray(fm)
    N = fm.size
    nt = M.node_type_of(fm)
    p = _tables(N, v, tables, seed=70 * N + v)
    sym = _symbols(N, v, B, N + v + L)
    if M.special_root(fm, kind):
        return _refused_on_both_sides(qpd, oracle_mod, kind, p, fm, nt, L, sym, engine)
    if ran is None:
        ran = FAST if engine != "generic" and _served_fast(kind, L) else GENERIC
    return _parity(qpd, oracle_mod, kind, p, fm, nt, L, sym, engine, ran, label)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("v", [16, 8])
@pytest.mark.parametrize("N,mask", MASKS)
@pytest.mark.parametrize("kind", KINDS)
def test_masks_match_oracle(kind, N, mask, v, engine, qpd, oracle_mod, monkeypatch):
    """Block and edge masks at L = 8, one quanta row per node and per element in turn.  all_info is the one
    root the Fast kinds refuse, on both sides."""
    _set_env(monkeypatch, {})
    fm = M.named_mask(N, mask)
    assert M.special_root(fm, kind) == (mask == "all_info" and kind.startswith("Fast"))
    tables = ("noderows", "ties")[MASKS.index((N, mask)) % 2]
    _mask_case(qpd, oracle_mod, kind, v, engine, fm, 8, 96, f"mask-{kind}-{N}-{mask}-v{v}-{engine}", tables=tables)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("v", [16, 8])
@pytest.mark.parametrize("N,K,seed", M.RANDOM_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_random_masks_match_oracle(kind, N, K, seed, v, engine, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    fm = M.random_mask(N, K, seed)
    assert not M.special_root(fm, kind)
    B = 48 if N >= 512 and "SCL" in kind else 96
    _mask_case(qpd, oracle_mod, kind, v, engine, fm, 8, B, f"mask-{kind}-{N}-random{seed}-v{v}-{engine}",
               tables=("noderows", "ties")[seed % 2])


L16_BLOCK = (64, 7)  # (N, block seed): R1 nodes of 32 and SPC of 16 elements


@pytest.mark.parametrize("v", [16, 8])
@pytest.mark.parametrize("kind,engine,ran", [("SCL-LUT", "auto", FAST), ("SCL-LUT", "generic", GENERIC),
                                             ("FastSCL-LUT", "fast", FAST), ("FastSCL-LUT", "auto", GENERIC)])
def test_block_mask_l16(kind, engine, ran, v, qpd, oracle_mod, monkeypatch):
    """L = 16 on a block mask: lane groups of 16 on the fast engine, FastSCL-LUT there on request."""
    _set_env(monkeypatch, {})
    N, seed = L16_BLOCK
    assert seed in M.BLOCK_SEEDS[N]
    _mask_case(qpd, oracle_mod, kind, v, engine, M.block_mask(N, seed), 16, 96,
               f"mask-l16-{kind}-block{seed}-v{v}-{engine}", ran)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("v", [16, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_block_mask_n1024(kind, v, engine, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    N = 1024
    fm = M.block_mask(N, M.BLOCK_SEEDS[N][0])
    assert not M.special_root(fm, kind)
    _mask_case(qpd, oracle_mod, kind, v, engine, fm, 8, 24, f"mask-{kind}-1024-block-v{v}-{engine}")


# ---------------------------------------------------------------------------------------------------------
# masks under the fast engine's schedule switches
# ---------------------------------------------------------------------------------------------------------

SWITCHES = [{"QPD_NO_PFX": "1"}, {"QPD_NO_PRE": "1"}, {"QPD_NO_BFUSE": "1"}, {"QPD_LDS_BUDGET": "256"}, {"QPD_SETS": "1"},
            {"QPD_SETS": "2"}]


@pytest.mark.parametrize("v", [16, 8])
@pytest.mark.parametrize("mask", [f"block{M.BLOCK_SEEDS[256][0]}", "info0", "frozen_last"])
@pytest.mark.parametrize("kind", KINDS)
def test_masks_under_schedule_switches(kind, mask, v, qpd, oracle_mod, monkeypatch):
    """The N = 256 block mask with the 64-element R1 node, an empty frozen prefix and a frozen last position
    under each schedule switch on its own (the switches are read when a decoder is created)."""
    N, L = 256, 8
    fm = M.named_mask(N, mask)
    nt = M.node_type_of(fm)
    K = int((fm == 0).sum())
    assert not M.special_root(fm, kind)
    if mask.startswith("block"):
        assert ("R1", 64) in M.labelled_nodes(fm)
    p = _tables(N, v, "noderows", seed=80 * N + v)
    sym = _symbols(N, v, 48, N + v)
    want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
    for env in SWITCHES:
        _set_env(monkeypatch, env)
        dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine="fast")
        assert dec.info()["engine"] == FAST
        assert_frames_equal(dec.decode_batch(sym), want, dec, f"mask-switch-{kind}-{mask}-v{v}-{'-'.join(env)}{''.join(env.values())}",
                            None, sym)


# ---------------------------------------------------------------------------------------------------------
# the CRC-aided kinds
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine,ran", [("auto", FAST), ("generic", GENERIC)])
@pytest.mark.parametrize("kind", ["CA-SCL-LUT", "CA-FastSCL-LUT"])
def test_ca_v8_block_mask(kind, engine, ran, qpd, oracle_mod, monkeypatch):
    """v = 8 on a block mask, frames that carry a real CRC (the code corrects some and not others, so the CRC
    check goes both ways; asserted for the oracle in test_oracle_alphabet_masks.py)."""
    from quantized_decoder_polar_codes_amd import lut as LU

    _set_env(monkeypatch, {})
    N, v, L = 256, 8, 8
    fm = M.block_mask(N, M.BLOCK_SEEDS[N][0])
    nt = M.node_type_of(fm)
    K = int((fm == 0).sum())
    A = K - 24
    p = LU.minsum_uniform_luts(N, v=v)
    msg, sym = M.ca_frames(oracle_mod.crc_encode, fm, A, 24, oracle_mod.CRC24_LOC, v, 96, seed=8)
    want = oracle_mod.decode_lut_ca(kind, p, K, A, L, fm, sym, node_type=nt)
    mk = lambda: qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine, A=A)  # noqa: E731
    dec = mk()
    assert dec.info()["engine"] == ran and dec.info()["out_bits"] == A
    got = dec.decode_batch(sym)
    assert_frames_equal(got, want, dec, f"ca-{kind}-v8-block-{engine}", lambda rows: mk().decode_batch(sym[rows]), sym)
    ok = (want == msg).all(1).mean()
    assert 0.0 < ok < 1.0
