"""The blind-detection metric on the kernel (qpd_dmetric / qpd_dmetric_host, include/qpd.h;
the DM twin of the float FastSC kernel, qpd_k_generic_dm.hip) and through the Python
surface (FastSCDecoder.dmetric_batch):

* the reference's own doubles (tests/golden/dmetric/dm_*.npz, DMetric.cpp:24-177) from a
  resident tensor and from host buffers forced onto the GPU, the bits decode_batch's;
* batch edges with canaries behind both outputs (the lanes clamped to frame B - 1 must
  not store), frames checked against tests/dmetric_ref.py;
* the metric alone (NULL bits), two streams on one handle, the kernel against the host
  engine on block masks, and the refusals.
Every metric is compared as the same double; no frame is left out.
"""
import ctypes
import glob
import os

import numpy as np
import pytest

import code_masks as M
import dmetric_ref
from conftest import GOLDEN_DIR, assert_engine, load_golden

pytestmark = pytest.mark.gpu

DM_FILES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "dmetric", "dm_*.npz")))
N32 = os.path.join(GOLDEN_DIR, "dmetric", "dm_pw_n32_k16.npz")
PAD = 64  # entries behind the B frames of a canaried buffer


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def fastsc(g):
    from quantized_decoder_polar_codes_amd.decoders import FastSCDecoder

    return FastSCDecoder(int(g["N"]), int(g["K"]), g["frozen"], 1 - g["frozen"], g["node_type"])


def tie_class_frames(N, B, seed):
    """B frames in the fixtures' three classes without a code's help: f % 3 == 0 a noisy all-zero
    codeword (of every linear code), 1 noise only, 2 LLRs from {-1, -0.5, 0, 0.5, 1}."""
    rng = np.random.default_rng(seed)
    noise = rng.normal(0, 0.9, size=(B, N))
    llr = (1.0 + noise) * 2 / 0.81
    cls = np.arange(B) % 3
    llr[cls == 1] = (noise * 2 / 0.81)[cls == 1]
    llr[cls == 2] = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])[rng.integers(0, 5, size=(B, N))][cls == 2]
    return np.ascontiguousarray(llr)


def dev_dmetric(dec, llr, bits=True, stream=None):
    """qpd_dmetric as a C caller on B resident frames: (metric, bits) device tensors PAD entries longer than
    B, pre-filled with canaries (metric -7.0, bits 0xEE)."""
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    t = llr if isinstance(llr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    B = t.shape[0]
    m = torch.full((B + PAD,), -7.0, dtype=torch.float64, device=t.device)
    out = torch.full((B + PAD, dec.out_bits), 0xEE, dtype=torch.uint8, device=t.device)
    _lib.check(_lib.load().qpd_dmetric(dec._h, ctypes.c_void_p(t.data_ptr()), B, ctypes.c_void_p(m.data_ptr()),
                                       ctypes.c_void_p(out.data_ptr()) if bits else None,
                                       ctypes.c_void_p(stream) if stream else None))
    torch.cuda.synchronize()
    return m.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("path", DM_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_kernel_reproduces_reference_dmetric(path, qpd):
    import torch

    g = load_golden(path)
    dec = fastsc(g)
    want_bits = dec.decode_batch(g["llr"])  # host buffers, on the kernels (QPD_HOST_ENGINE=gpu here)
    assert_engine(dec, "gpu")
    assert (want_bits == dmetric_ref.dmetric(int(g["N"]), g["frozen"], g["node_type"], g["llr"])[1]).all()
    # a resident tensor: qpd_dmetric on the current stream
    x = torch.from_numpy(g["llr"]).cuda()
    m, bits = dec.dmetric_batch(x, return_bits=True)
    assert m.is_cuda and m.dtype == torch.float64 and bits.is_cuda
    assert (m.cpu().numpy() == g["dmetric"]).all(), np.flatnonzero(m.cpu().numpy() != g["dmetric"])
    assert (bits.cpu().numpy() == want_bits).all()
    assert_engine(dec, "gpu")
    m1 = dec.dmetric_batch(x)
    assert (m1.cpu().numpy() == g["dmetric"]).all()
    # host buffers: qpd_dmetric_host forced onto the GPU
    mh, bh = dec.dmetric_batch(g["llr"], return_bits=True)
    assert_engine(dec, "gpu")
    assert isinstance(mh, np.ndarray) and (mh == g["dmetric"]).all() and (bh == want_bits).all()
    assert (dec.dmetric_batch(g["llr"]) == g["dmetric"]).all()  # no bits: nothing copied back for them
    assert (dec.dmetric_batch(torch.from_numpy(g["llr"])) == g["dmetric"]).all()  # a CPU tensor
    # other float dtypes are converted as decode_batch converts them
    x32 = g["llr"][2::3].astype(np.float32)  # the tie class is exact in float32
    assert (dec.dmetric_batch(torch.from_numpy(x32).cuda()).cpu().numpy() == g["dmetric"][2::3]).all()


@pytest.fixture(scope="module")
def edge_case(qpd):
    """The N = 32 fixture's code, 130 frames made here and their reference result, once."""
    g = load_golden(N32)
    llr = tie_class_frames(32, 130, 77)
    dec = fastsc(g)
    dec.set_host_engine("gpu")  # (created before a test's QPD_HOST_ENGINE is set: module scope)
    return g, dec, llr, dmetric_ref.dmetric(32, g["frozen"], g["node_type"], llr)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_batch_edges_leave_the_tail_untouched(B, edge_case):
    g, dec, llr, (want_m, want_bits) = edge_case
    m, bits = dev_dmetric(dec, llr[:B])
    assert_engine(dec, "gpu")
    assert (m[:B] == want_m[:B]).all() and (bits[:B] == want_bits[:B]).all()
    assert (m[B:] == -7.0).all() and (bits[B:] == 0xEE).all()  # the clamped lanes did not store
    # the metric alone: the same doubles, and the bit buffer is not touched at all
    m0, bits0 = dev_dmetric(dec, llr[:B], bits=False)
    assert (m0[:B] == want_m[:B]).all() and (m0[B:] == -7.0).all() and (bits0 == 0xEE).all()
    # through host buffers
    mh = np.full(B + PAD, -7.0)
    bh = np.full((B + PAD, dec.out_bits), 0xEE, dtype=np.uint8)
    from quantized_decoder_polar_codes_amd import _lib

    x = np.ascontiguousarray(llr[:B])
    _lib.check(_lib.load().qpd_dmetric_host(dec._h, x.ctypes.data, B, mh.ctypes.data, bh.ctypes.data))
    assert_engine(dec, "gpu")
    assert (mh[:B] == want_m[:B]).all() and (bh[:B] == want_bits[:B]).all()
    assert (mh[B:] == -7.0).all() and (bh[B:] == 0xEE).all()


def test_two_streams_on_one_handle(edge_case):
    import torch

    g, dec, llr, (want_m, want_bits) = edge_case
    a = torch.from_numpy(llr).cuda()
    b = torch.from_numpy(np.ascontiguousarray(llr[::-1])).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(side):
            m = dec.dmetric_batch(a)
        bits = dec.decode_batch(b)  # the default stream, the same handle and slab
        torch.cuda.synchronize()
        assert (m.cpu().numpy() == want_m).all()
        assert (bits.cpu().numpy() == want_bits[::-1]).all()


@pytest.mark.host_engine
@pytest.mark.parametrize("N,seed", [(64, M.BLOCK_SEEDS[64][0]), (256, M.BLOCK_SEEDS[256][0])])
def test_kernel_equals_host_engine_on_block_masks(N, seed, qpd):
    from quantized_decoder_polar_codes_amd.decoders import FastSCDecoder

    fm = M.block_mask(N, seed)
    assert not M.special_root(fm, "FastSC-LUT")
    nt = M.node_type_of(fm)
    assert {"R0", "REP"} <= {k for k, s in M.labelled_nodes(fm) if s > 1}
    llr = tie_class_frames(N, 96, N + seed)
    dec = FastSCDecoder(N, int((fm == 0).sum()), fm, 1 - fm, nt)
    dec.set_host_engine("cpu")
    mc, bc = dec.dmetric_batch(llr, return_bits=True)
    assert_engine(dec, "host")
    dec.set_host_engine("gpu")
    mg, bg = dec.dmetric_batch(llr, return_bits=True)
    assert_engine(dec, "gpu")
    want_m, want_bits = dmetric_ref.dmetric(N, fm, nt, llr)
    assert (mg == mc).all() and (bg == bc).all()
    assert (mg == want_m).all() and (bg == want_bits).all()


def test_wrong_kind_is_refused_before_any_launch(qpd):
    import torch

    from quantized_decoder_polar_codes_amd import _lib
    from quantized_decoder_polar_codes_amd import decoders as D
    from quantized_decoder_polar_codes_amd import lut as LU

    g = load_golden(N32)
    N, K = 32, int(g["K"])
    scl = D.SCLDecoder(N, K, 4, g["frozen"], 1 - g["frozen"])
    sclut = D.from_packed("SC-LUT", LU.random_luts(N, 16, seed=5), K, g["frozen"])
    x = torch.from_numpy(g["llr"]).cuda()
    for dec, name in ((scl, "SCLDecoder"), (sclut, "SCLUTDecoder")):
        with pytest.raises(TypeError, match="FastSCDecoder"):  # Python, before the C call
            dec.dmetric_batch(x)
        before = dec.info()["last_engine"]
        m = torch.full((len(x),), -7.0, dtype=torch.float64, device="cuda")
        L = _lib.load()
        rc = L.qpd_dmetric(dec._h, ctypes.c_void_p(x.data_ptr()), len(x), ctypes.c_void_p(m.data_ptr()), None, None)
        assert rc == _lib.QPD_E_INVALID and name in L.qpd_last_error().decode()
        mh = np.full(len(x), -7.0)
        rc = L.qpd_dmetric_host(dec._h, g["llr"].ctypes.data, len(x), mh.ctypes.data, None)
        assert rc == _lib.QPD_E_INVALID and name in L.qpd_last_error().decode()
        torch.cuda.synchronize()
        assert dec.info()["last_engine"] == before == _lib.QPD_RAN_NONE  # nothing ran
        assert (m.cpu().numpy() == -7.0).all() and (mh == -7.0).all()
    # a NULL metric on the right kind
    dec = fastsc(g)
    rc = _lib.load().qpd_dmetric(dec._h, ctypes.c_void_p(x.data_ptr()), len(x), None, None, None)
    assert rc == _lib.QPD_E_INVALID and dec.info()["last_engine"] == _lib.QPD_RAN_NONE
