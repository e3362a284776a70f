"""uint8 channel symbols on the GPU: qpd_decode_u8 / qpd_decode_u8_host through the ctypes binding, against
the CPU oracle and against the same decoder's int32 call on the same symbols.

Two ways in (qpd_info.u8_staged says which one a call took):

* direct (0): a fast-engine decoder in pre-mode -- root_pre_kernel<uint8_t> reads the bytes, eight per 64-bit
  load with a SWAR range check and nibble pack where the buffer is 8-byte aligned, a rolled byte loop where
  it is not; everything after its rows is the int32 path's;
* staged (1): every other decoder widens a chunk of frames into its own int32 buffer (widen_u8_kernel) and
  runs the int32 launch on it.

B = 97 in most cases: the last pre-pass block is partial and the last wave task short.  Every case asserts
the engine the decoder was built on, the engine that ran and u8_staged."""
import ctypes

import numpy as np
import pytest

import code_masks as M
from conftest import assert_frames_equal

pytestmark = pytest.mark.gpu

ENV = ("QPD_NO_PFX", "QPD_NO_PRE", "QPD_NO_BFUSE", "QPD_LDS_BUDGET", "QPD_SETS", "QPD_PFX1B", "QPD_PRE_CHUNK",
       "QPD_U8_CHUNK")
FAST, GENERIC = 2, 1  # qpd_info.engine
RAN_GPU, RAN_HOST = 1, 2  # qpd_info.last_engine
B97 = 97


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


def _tables(N, v, seed, **kw):
    from quantized_decoder_polar_codes_amd import lut as LU

    return LU.random_luts(N, v, seed=seed, distinct_mags=3, **kw)


def _symbols(N, v, B, seed):
    sym = np.random.default_rng(seed).integers(0, v, size=(B, N), dtype=np.int32)
    sym[0, :2] = (0, v - 1)  # both ends of the alphabet
    return sym


# -- the binding, called as a C caller would --------------------------------------------------------------

def _rc_dev(dec, name, t, B=None, out=None, stream=None):
    """Return code of qpd_decode / qpd_decode_u8 on the device tensor t (and the output tensor)."""
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    B = t.shape[0] if B is None else B
    if out is None:
        out = torch.empty((max(B, 1), dec.out_bits), dtype=torch.uint8, device=t.device)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = getattr(_lib.load(), name)(dec._h, ctypes.c_void_p(t.data_ptr()), B, ctypes.c_void_p(out.data_ptr()),
                                    ctypes.c_void_p(st))
    return rc, out


def dev_u8(dec, t):
    from quantized_decoder_polar_codes_amd import _lib

    import torch

    assert t.dtype == torch.uint8 and t.is_contiguous()
    rc, out = _rc_dev(dec, "qpd_decode_u8", t)
    _lib.check(rc)
    return out


def dev_i32(dec, t):
    from quantized_decoder_polar_codes_amd import _lib

    import torch

    assert t.dtype == torch.int32 and t.is_contiguous()
    rc, out = _rc_dev(dec, "qpd_decode", t)
    _lib.check(rc)
    return out


def host_u8(dec, a):
    from quantized_decoder_polar_codes_amd import _lib

    a = np.ascontiguousarray(a, dtype=np.uint8)
    out = np.empty((len(a), dec.out_bits), dtype=np.uint8)
    _lib.check(_lib.load().qpd_decode_u8_host(dec._h, a.ctypes.data, len(a), out.ctypes.data))
    return out


def input_error(dec):
    """qpd_check_input_error's return code (waits for the decoder's work, clears the flag)."""
    from quantized_decoder_polar_codes_amd import _lib

    return _lib.load().qpd_check_input_error(dec._h)


def _state(dec):
    i = dec.info()
    return i["engine"], i["last_engine"], i["u8_staged"]


def _check(dec, sym, want, engine, staged, label):
    """uint8 device call, int32 device call and uint8 host-buffer call (on the kernels: conftest's fixture)
    on the same symbols: the oracle's bits from each, and the state each call leaves in qpd_info."""
    import torch

    t32 = torch.from_numpy(sym).cuda()
    t8 = t32.to(torch.uint8)
    got8 = dev_u8(dec, t8).cpu().numpy()
    assert _state(dec) == (engine, RAN_GPU, staged), (label, _state(dec))
    assert input_error(dec) == 0
    got32 = dev_i32(dec, t32).cpu().numpy()
    assert _state(dec) == (engine, RAN_GPU, 0), (label, _state(dec))
    goth = host_u8(dec, sym)
    assert _state(dec) == (engine, RAN_GPU, staged), (label, _state(dec))
    assert_frames_equal(got8, want, dec, f"u8-{label}", None, sym)
    assert_frames_equal(got32, want, dec, f"u8-i32-{label}", None, sym)
    assert_frames_equal(goth, want, dec, f"u8-host-{label}", None, sym)
    assert (got8 == got32).all()


def _lut_case(qpd, oracle_mod, kind, N, K, L, v, engine, ran, staged, label, fm=None, nt=None, B=B97, tables=None,
              sym=None):
    if fm is None:
        fm, nt = _pw(N, K)
    K = int((np.asarray(fm) == 0).sum())
    p = _tables(N, v, seed=31 * N + v + L) if tables is None else tables
    sym = _symbols(N, v, B, N + v + L) if sym is None else sym
    if kind.startswith("CA-"):
        A = K - 4 if N == 16 else K - 24
        want = oracle_mod.decode_lut_ca(kind, p, K, A, L, fm, sym, node_type=nt)
        dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine, A=A)
    else:
        want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
        dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine)
    assert dec.info()["engine"] == ran, (label, dec.info()["engine"])
    _check(dec, sym, want, ran, staged, label)
    return dec


# ---------------------------------------------------------------------------------------------------------
# direct path: the byte-reading root pre-pass
# ---------------------------------------------------------------------------------------------------------

# (16, 10): the left half holds three information positions, so no Fast kind labels the root's left child
# (at K = 8 it is a REP node, and FastSCL-LUT has no pre-pass)
DIRECT_SHAPES = [(16, 10), (128, 64)]
DIRECT_KINDS = [("SC-LUT", 1), ("SCL-LUT", 8), ("FastSCL-LUT", 8), ("CA-SCL-LUT", 8)]


@pytest.mark.parametrize("v", [2, 8, 15, 16])
@pytest.mark.parametrize("N,K", DIRECT_SHAPES)
@pytest.mark.parametrize("kind,L", DIRECT_KINDS)
def test_direct_matches_oracle_and_int32(kind, L, N, K, v, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    _lut_case(qpd, oracle_mod, kind, N, K, L, v, "auto", FAST, 0, f"direct-{kind}-{N}-v{v}")


@pytest.mark.parametrize("v", [2, 8, 15, 16])
def test_direct_l16(v, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    _lut_case(qpd, oracle_mod, "SCL-LUT", 128, 64, 16, v, "auto", FAST, 0, f"direct-l16-v{v}")


def test_direct_n1024(qpd, oracle_mod, monkeypatch):
    """64 output words per half and frame: a wave's 64 threads read 512 consecutive bytes of each half."""
    _set_env(monkeypatch, {})
    _lut_case(qpd, oracle_mod, "SCL-LUT", 1024, 512, 8, 16, "auto", FAST, 0, "direct-n1024")


@pytest.mark.parametrize("kind,L", [("SC-LUT", 1), ("SCL-LUT", 8)])
def test_direct_chunk_seams(kind, L, qpd, oracle_mod, monkeypatch):
    """QPD_PRE_CHUNK = 32 at B = 97: four pre-pass launches, the input and output offsets of each chunk."""
    _set_env(monkeypatch, {"QPD_PRE_CHUNK": "32"})
    dec = _lut_case(qpd, oracle_mod, kind, 128, 64, L, 16, "auto", FAST, 0, f"direct-seams-{kind}")
    dec.profile(True)
    import torch

    dev_u8(dec, torch.zeros((B97, 128), dtype=torch.uint8, device="cuda"))
    assert dec.kernel_times()["pre"][1] == 4


@pytest.mark.parametrize("N,K", DIRECT_SHAPES)
@pytest.mark.parametrize("v", [8, 16])
def test_direct_unaligned_input(N, K, v, qpd, oracle_mod, monkeypatch):
    """A row base one byte into the storage (odd: the rolled byte reader) and one at 8-byte but not 16-byte
    alignment (the 64-bit loads): the same bits as from the aligned tensor."""
    import torch

    _set_env(monkeypatch, {})
    L = 8
    fm, nt = _pw(N, K)
    p = _tables(N, v, seed=5 * N + v)
    sym = _symbols(N, v, B97, N + v)
    want = oracle_mod.decode_lut("SCL-LUT", p, K, L, fm, sym)
    dec = qpd.from_packed("SCL-LUT", p, K, fm, L=L)
    store = torch.zeros(B97 * N + 64, dtype=torch.uint8, device="cuda")
    assert store.data_ptr() % 16 == 0
    flat = torch.from_numpy(sym.astype(np.uint8)).cuda().reshape(-1)
    for off in (1, 8, 0):
        t = store[off: off + B97 * N]
        t.copy_(flat)
        t = t.view(B97, N)
        assert t.is_contiguous() and t.data_ptr() % 16 == off
        got = dev_u8(dec, t).cpu().numpy()
        assert _state(dec) == (FAST, RAN_GPU, 0)
        assert input_error(dec) == 0
        assert_frames_equal(got, want, dec, f"u8-unaligned-{N}-v{v}-off{off}", None, sym)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("value", [8, 16, 200])
def test_direct_range_check(value, off, qpd, oracle_mod, monkeypatch):
    """At v = 8 one symbol of one frame is 8 (fits the nibble), 16 (low nibble in range, high nibble set) or
    200, in the root's first half and in its second, read by the 64-bit reader (off 0) and by the rolled one
    (off 1): reported by the host call and, after the device call, by qpd_check_input_error; the flag is
    clear afterwards and the next clean batch decodes to the oracle's bits."""
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    _set_env(monkeypatch, {})
    N, K, L, v = 128, 64, 4, 8
    fm, nt = _pw(N, K)
    p = _tables(N, v, seed=61)
    sym = _symbols(N, v, B97, 62).astype(np.uint8)
    want = oracle_mod.decode_lut("SCL-LUT", p, K, L, fm, sym.astype(np.int32))
    dec = qpd.from_packed("SCL-LUT", p, K, fm, L=L)
    assert dec.info()["engine"] == FAST
    store = torch.zeros(B97 * N + 16, dtype=torch.uint8, device="cuda")

    def on_device(a):
        t = store[off: off + B97 * N].view(B97, N)
        t.copy_(torch.from_numpy(a).cuda())
        assert t.data_ptr() % 8 == off
        return dev_u8(dec, t)

    for pos in (5, N // 2 + 5):
        bad = sym.copy()
        bad[17, pos] = value
        if off == 0:
            with pytest.raises(ValueError, match="outside"):
                host_u8(dec, bad)
            assert input_error(dec) == 0  # the host call reported and cleared it
        on_device(bad)
        assert input_error(dec) == _lib.QPD_E_INPUT
        assert input_error(dec) == 0
        assert _state(dec) == (FAST, RAN_GPU, 0)
        got = on_device(sym).cpu().numpy()
        assert input_error(dec) == 0
        assert_frames_equal(got, want, dec, f"u8-range-{value}-{off}-{pos}", None, sym)


# ---------------------------------------------------------------------------------------------------------
# staged path: widen, then the int32 launch
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,L", [("SC-LUT", 1), ("SCL-LUT", 4)])
def test_staged_n8(kind, L, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    _lut_case(qpd, oracle_mod, kind, 8, 4, L, 16, "auto", FAST, 1, f"staged-n8-{kind}")


def test_staged_no_pre(qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {"QPD_NO_PRE": "1"})
    _lut_case(qpd, oracle_mod, "SCL-LUT", 128, 64, 8, 16, "auto", FAST, 1, "staged-nopre")


def test_staged_special_left_child(qpd, oracle_mod, monkeypatch):
    """antipolar: the root's left child is one R1 node, so FastSCL-LUT runs the root's f on the channel."""
    _set_env(monkeypatch, {})
    N = 64
    fm = M.named_mask(N, "antipolar")
    assert M.labelled_nodes(fm)[0] == ("R1", N // 2) and not M.special_root(fm, "FastSCL-LUT")
    _lut_case(qpd, oracle_mod, "FastSCL-LUT", N, None, 8, 16, "auto", FAST, 1, "staged-antipolar", fm=fm,
              nt=M.node_type_of(fm))


def test_staged_generic_v16(qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    _lut_case(qpd, oracle_mod, "SCL-LUT", 128, 64, 8, 16, "generic", GENERIC, 1, "staged-generic-v16")


@pytest.mark.parametrize("v,N", [(17, 128), (256, 32)])
def test_staged_wide_alphabet(v, N, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    sym = _symbols(N, v, B97, N + v)
    assert (sym == v - 1).any()
    _lut_case(qpd, oracle_mod, "SCL-LUT", N, N // 2, 8, v, "auto", GENERIC, 1, f"staged-v{v}", sym=sym)


def test_staged_per_element_tables_v8(qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    N, v = 64, 8
    _lut_case(qpd, oracle_mod, "SC-LUT", N, 32, 1, v, "auto", GENERIC, 1, "staged-perelem",
              tables=_tables(N, v, seed=77, per_element=True))


def test_staged_l32(qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    _lut_case(qpd, oracle_mod, "SCL-LUT", 128, 64, 32, 16, "auto", GENERIC, 1, "staged-l32", B=48)


@pytest.mark.parametrize("N,K,engine,ran", [(128, 64, "generic", GENERIC), (8, 4, "auto", FAST)])
def test_staged_two_chunks(N, K, engine, ran, qpd, oracle_mod, monkeypatch):
    """QPD_U8_CHUNK = 40 frames (read when the decoder is created) at B = 97: three staging chunks through
    one 40-frame buffer, each widened after the decode of the one before on the same stream."""
    _set_env(monkeypatch, {"QPD_U8_CHUNK": "40"})
    dec = _lut_case(qpd, oracle_mod, "SCL-LUT", N, K, 4, 16, engine, ran, 1, f"staged-chunks-{N}")
    dec.profile(True)
    import torch

    dev_u8(dec, torch.zeros((B97, N), dtype=torch.uint8, device="cuda"))
    assert dec.kernel_times()["decode"][1] == 3


# ---------------------------------------------------------------------------------------------------------
# the host-buffer call's dispatch
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.host_engine
@pytest.mark.parametrize("engine,ran,staged", [("auto", FAST, 0), ("generic", GENERIC, 1)])
def test_host_buffer_dispatch(engine, ran, staged, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    monkeypatch.delenv("QPD_HOST_ENGINE", raising=False)
    N, K, L, v = 128, 64, 4, 8
    fm, nt = _pw(N, K)
    p = _tables(N, v, seed=88)
    dec = qpd.from_packed("SCL-LUT", p, K, fm, L=L, engine=engine)
    hm = dec.info()["host_max_frames"]
    assert 1 <= hm < 4096
    sym = _symbols(N, v, hm + 1, 89).astype(np.uint8)
    want = oracle_mod.decode_lut("SCL-LUT", p, K, L, fm, sym.astype(np.int32))
    for B, engine_ran, st in ((1, RAN_HOST, 0), (hm, RAN_HOST, 0), (hm + 1, RAN_GPU, staged)):
        got = host_u8(dec, sym[:B])
        assert _state(dec) == (ran, engine_ran, st), (B, _state(dec))
        assert_frames_equal(got, want[:B], dec, f"u8-hostbuf-{engine}-{B}", None, sym, engine=None)
    bad = sym[:1].copy()
    bad[0, N // 2] = v
    with pytest.raises(ValueError, match="outside"):  # the host engine's own range test on bytes
        host_u8(dec, bad)
    assert dec.info()["last_engine"] == RAN_HOST
    dec.set_host_engine("gpu")
    got = host_u8(dec, sym[:1])
    assert _state(dec) == (ran, RAN_GPU, staged)
    assert_frames_equal(got, want[:1], dec, f"u8-hostbuf-{engine}-gpu", None, sym)


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------

def test_refusals(qpd, monkeypatch):
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    _set_env(monkeypatch, {})
    lib = _lib.load()
    N, K = 64, 32
    fm, nt = _pw(N, K)
    t = torch.zeros((4, N), dtype=torch.uint8, device="cuda")
    a = np.zeros((4, N), dtype=np.uint8)
    out = np.zeros((4, K), dtype=np.uint8)
    flt = qpd.SCDecoder(N, K, fm, 1 - fm)
    assert _rc_dev(flt, "qpd_decode_u8", t)[0] == _lib.QPD_E_INVALID
    assert b"float64" in lib.qpd_last_error()
    assert lib.qpd_decode_u8_host(flt._h, a.ctypes.data, 4, out.ctypes.data) == _lib.QPD_E_INVALID
    assert b"float64" in lib.qpd_last_error()
    dec = qpd.from_packed("SC-LUT", _tables(N, 16, seed=3), K, fm)
    null = ctypes.c_void_p(None)
    o = torch.zeros((4, K), dtype=torch.uint8, device="cuda")
    for name, dev in (("qpd_decode_u8", True), ("qpd_decode", True), ("qpd_decode_u8_host", False),
                      ("qpd_decode_host", False)):
        fn = getattr(lib, name)
        i_p = ctypes.c_void_p(t.data_ptr() if dev else a.ctypes.data)
        o_p = ctypes.c_void_p(o.data_ptr() if dev else out.ctypes.data)
        tail = (null,) if dev else ()
        assert fn(dec._h, null, 4, o_p, *tail) == _lib.QPD_E_INVALID, name
        assert fn(dec._h, i_p, 4, null, *tail) == _lib.QPD_E_INVALID, name
        assert fn(dec._h, i_p, -1, o_p, *tail) == _lib.QPD_E_INVALID, name
        assert fn(dec._h, null, 0, null, *tail) == _lib.QPD_OK, name
        assert fn(null, i_p, 4, o_p, *tail) == _lib.QPD_E_INVALID, name
    assert dec.info()["last_engine"] == 0  # nothing ran


# ---------------------------------------------------------------------------------------------------------
# decode_batch
# ---------------------------------------------------------------------------------------------------------

class _Spy:
    """Counts the calls of one entry point of the loaded library."""

    def __init__(self, monkeypatch, name):
        from quantized_decoder_polar_codes_amd import _lib

        lib = _lib.load()
        self.fn, self.calls = getattr(lib, name), 0
        monkeypatch.setattr(lib, name, self)

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def test_decode_batch_dtype_rule(qpd, oracle_mod, monkeypatch):
    """torch.uint8 on the device goes to qpd_decode_u8 as it is (no int32 copy: the allocator's peak grows by
    less than B * N * 4 bytes), numpy / CPU-tensor uint8 to qpd_decode_u8_host; int8 keeps the int32 path."""
    import torch

    _set_env(monkeypatch, {})
    N, K, L, v, B = 128, 64, 8, 16, B97
    fm, nt = _pw(N, K)
    p = _tables(N, v, seed=12)
    sym = _symbols(N, v, B, 13)
    want = oracle_mod.decode_lut("SCL-LUT", p, K, L, fm, sym)
    dec = qpd.from_packed("SCL-LUT", p, K, fm, L=L)
    gen = qpd.from_packed("SCL-LUT", p, K, fm, L=L, engine="generic")
    u8d, u8h = _Spy(monkeypatch, "qpd_decode_u8"), _Spy(monkeypatch, "qpd_decode_u8_host")
    t8 = torch.from_numpy(sym.astype(np.uint8)).cuda()
    ref = dec.decode_batch(t8.to(torch.int32))
    assert (u8d.calls, u8h.calls) == (0, 0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = dec.decode_batch(t8)
    grown = torch.cuda.max_memory_allocated() - before
    assert (u8d.calls, u8h.calls) == (1, 0)
    assert _state(dec) == (FAST, RAN_GPU, 0)
    assert got.dtype == torch.uint8 and torch.equal(got, ref)
    assert B * dec.out_bits <= grown < B * N * 4, grown
    assert_frames_equal(got.cpu().numpy(), want, dec, "u8-batch-torch", None, sym)
    # numpy and CPU-tensor uint8: the host entry point, no device tensor at all
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for x in (sym.astype(np.uint8), torch.from_numpy(sym.astype(np.uint8))):
        goth = dec.decode_batch(x)
        assert _state(dec) == (FAST, RAN_GPU, 0)
        assert_frames_equal(goth, want, dec, "u8-batch-numpy", None, sym)
    assert (u8d.calls, u8h.calls) == (1, 2)
    assert torch.cuda.max_memory_allocated() - before < B * N * 4
    # the generic decoder shows which entry point a call took: uint8 is staged, int8 and bool are not
    assert_frames_equal(gen.decode_batch(sym.astype(np.uint8)), want, gen, "u8-batch-generic", None, sym)
    assert _state(gen) == (GENERIC, RAN_GPU, 1) and u8h.calls == 3
    for x in (sym.astype(np.int8), torch.from_numpy(sym.astype(np.int8)).cuda()):
        g = gen.decode_batch(x)
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        assert _state(gen) == (GENERIC, RAN_GPU, 0)
        assert_frames_equal(g, want, gen, "i8-batch-generic", None, sym)
    ones = (sym & 1).astype(bool)
    assert (gen.decode_batch(ones) == gen.decode_batch(ones.astype(np.int32))).all()
    assert _state(gen) == (GENERIC, RAN_GPU, 0)
    assert (u8d.calls, u8h.calls) == (1, 3)
    # the per-frame call stays on int32
    one = dec.decode(sym[0].astype(np.uint8))
    assert (one == want[0]).all() and (u8d.calls, u8h.calls) == (1, 3)


# ---------------------------------------------------------------------------------------------------------
# stream ordering
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine,ran,staged", [("auto", FAST, 0), ("generic", GENERIC, 1)])
def test_u8_then_i32_on_two_streams(engine, ran, staged, qpd, oracle_mod, monkeypatch):
    """A uint8 call on one stream, an int32 call on another right behind it, no host synchronization in
    between: the staging buffer, the pre-pass rows and the slab are the handle's, so the second waits."""
    import torch

    _set_env(monkeypatch, {})
    N, K = 128, 32
    fm, nt = _pw(N, K)
    p = _tables(N, 16, seed=21)
    B = 1 << 12
    sa, sb = _symbols(N, 16, B, 22), _symbols(N, 16, B, 23)
    dec = qpd.from_packed("SC-LUT", p, K, fm, engine=engine)
    ta, tb = torch.from_numpy(sa.astype(np.uint8)).cuda(), torch.from_numpy(sb).cuda()
    seq_a, seq_b = dev_u8(dec, ta), dev_i32(dec, tb)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    oa, ob = torch.empty_like(seq_a), torch.empty_like(seq_b)
    rc1, _ = _rc_dev(dec, "qpd_decode_u8", ta, out=oa, stream=s1.cuda_stream)
    assert dec.info()["u8_staged"] == staged
    rc2, _ = _rc_dev(dec, "qpd_decode", tb, out=ob, stream=s2.cuda_stream)
    assert (rc1, rc2) == (0, 0)
    assert _state(dec) == (ran, RAN_GPU, 0)
    torch.cuda.synchronize()
    assert torch.equal(oa, seq_a) and torch.equal(ob, seq_b)
    assert_frames_equal(oa.cpu().numpy(), oracle_mod.decode_lut("SC-LUT", p, K, 1, fm, sa), dec, f"u8-streams-a-{engine}")
    assert_frames_equal(ob.cpu().numpy(), oracle_mod.decode_lut("SC-LUT", p, K, 1, fm, sb), dec, f"u8-streams-b-{engine}")
