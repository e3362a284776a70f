"""tests/dmetric_ref.py, the checker of the blind-detection metric tests, against the
reference's own doubles (tests/golden/dmetric/dm_*.npz, recorded from
DMetricCalculator::calculate by tests/golden/make_dmetric_golden.py): the same double
on every frame of every fixture, no tolerance and no frame left out."""
import glob
import os

import numpy as np
import pytest

import dmetric_ref
from conftest import GOLDEN_DIR, golden_files, load_golden
from quantized_decoder_polar_codes_amd import codes as C

DM_FILES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "dmetric", "dm_*.npz")))


def test_fixtures_are_the_four_and_informative():
    assert [os.path.basename(p)[:-4] for p in DM_FILES] == ["dm_block_n256_k104", "dm_pw_n128_k64", "dm_pw_n256_k50",
                                                             "dm_pw_n32_k16"]
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
    for path in DM_FILES:
        g = load_golden(path)
        N = int(g["N"])
        assert g["llr"].shape == (48, N) and g["dmetric"].shape == (48,) and np.isfinite(g["llr"]).all()
        assert int((g["frozen"] == 0).sum()) == int(g["K"])
        assert (g["node_type"] == C.identify_nodes(N, np.flatnonzero(g["frozen"] == 0)).astype(np.int32)).all()
        ties = g["llr"][2::3]  # the tie class: only the five values
        assert np.isin(ties, [-1.0, -0.5, 0.0, 0.5, 1.0]).all() and not np.isin(g["llr"][0::3], [0.0]).any()
        assert os.path.getsize(path) <= biggest
    # conftest.golden_files() must not hand them to the plain decoders' tests
    assert not [p for p in golden_files() + golden_files("float_*.npz") if os.path.basename(p).startswith("dm_")]


@pytest.mark.parametrize("path", DM_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_reproduces_the_reference_doubles(path):
    g = load_golden(path)
    dm, bits = dmetric_ref.dmetric(int(g["N"]), g["frozen"], g["node_type"], g["llr"])
    assert dm.dtype == np.float64 and (dm == g["dmetric"]).all(), np.flatnonzero(dm != g["dmetric"])
    assert bits.shape == (48, int(g["K"]))
    # one frame at a time gives the same doubles (the batch axis is only side by side)
    one = np.array([dmetric_ref.dmetric(int(g["N"]), g["frozen"], g["node_type"], x)[0][0] for x in g["llr"][:6]])
    assert (one == g["dmetric"][:6]).all()
