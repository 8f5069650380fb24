"""The one-top Data layer (CPU and GPU, LMDB and synthetic feed) and the
gaussian filler's `sparse` (filler.hpp:109-125)."""
import os
import sys

import numpy as np
import pytest

import caffe_amd as ca
from engine_util import REPO, net_from_text

sys.path.insert(0, os.path.join(REPO, "tools"))
from make_lmdb import make_lmdb  # noqa: E402

MODES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
N_REC, C, H, W = 12, 1, 6, 5


@pytest.fixture(autouse=True)
def reset_stream():
    ca.set_data_iter(0)
    ca.set_rank_world(0, 1)
    yield
    ca.set_data_iter(0)
    ca.set_mode("cpu")


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    d = tmp_path_factory.mktemp("ae_lmdb") / "db"
    make_lmdb(str(d), N_REC, C, H, W, 31)
    return str(d)


def data_net(tops, source=None):
    src = f'source: "{source}" backend: LMDB' if source else ""
    top_txt = " ".join(f'top: "{t}"' for t in tops)
    return net_from_text(f"""name: "d"
layer {{ name: "data" type: "Data" {top_txt}
  data_param {{ {src} batch_size: 5 }}
  transform_param {{ scale: 0.0039215684 }} }}
""")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("feed", ["lmdb", "synthetic"])
def test_one_top_data_equals_two_top_data(db, mode, feed):
    ca.set_mode(mode)
    ca.set_synthetic_shape(C, H, W, 10)
    source = db if feed == "lmdb" else None
    one = data_net(["data"], source)
    two = data_net(["data", "label"], source)
    assert one.blob_names() == ["data"]
    for it in range(4):  # 4 x 5 records: wraps the 12-record database
        ca.set_data_iter(it)
        one.forward()
        ca.set_data_iter(it)
        two.forward()
        a, b = one.blob("data"), two.blob("data")
        assert a.shape == (5, C, H, W)
        assert np.array_equal(a, b)
        if feed == "lmdb":
            # uint8 pixels scaled by 1/255: valid cross-entropy targets
            assert a.min() >= 0.0 and a.max() <= 1.0 and a.max() > 0.5
    assert two.blob("label").shape == (5,)


def test_three_tops_is_an_error():
    ca.set_mode("cpu")
    ca.set_synthetic_shape(C, H, W, 10)
    with pytest.raises(ca.CaffeError, match="at most 2"):
        data_net(["data", "label", "extra"])


# ------------------------------------------------------------------ filler
def ip_net(filler, nout=200, nin=300):
    return net_from_text(f"""name: "f"
layer {{ name: "in" type: "Input" top: "x"
  input_param {{ shape {{ dim: 1 dim: {nin} }} }} }}
layer {{ name: "ip" type: "InnerProduct" bottom: "x" top: "y"
  inner_product_param {{ num_output: {nout} bias_term: false
    weight_filler {{ {filler} }} }} }}
""")


def test_gaussian_sparse_mask():
    ca.set_mode("cpu")
    ca.set_random_seed(77)
    w = ip_net('type: "gaussian" std: 2 sparse: 15').param(0)
    assert w.size == 60000
    nz = int(np.count_nonzero(w))
    # Bernoulli(p = sparse / shape(0) = 15 / 200): n = 60000, p = 0.075,
    # mean 4500, sigma = sqrt(n p (1 - p)) = 64.5; six sigma
    assert abs(nz - 4500) <= 6 * 64.5, nz
    # the survivors are the gaussian's values: std 2 +- 6 standard errors
    # (the standard error of a sample std is sigma / sqrt(2 n))
    kept = w[w != 0]
    assert abs(kept.std() - 2.0) <= 6 * 2.0 / np.sqrt(2 * kept.size)
    assert abs(kept.mean()) <= 6 * 2.0 / np.sqrt(kept.size)
    # per output row the mean number of non-zeros is sparse * nin / nout
    per_row = np.count_nonzero(w.reshape(200, 300), axis=1)
    assert abs(per_row.mean() - 22.5) < 1.0


def test_sparse_zero_and_dense():
    ca.set_mode("cpu")
    assert np.count_nonzero(
        ip_net('type: "gaussian" std: 1 sparse: 0').param(0)) == 0
    assert np.count_nonzero(
        ip_net('type: "gaussian" std: 1 sparse: 200').param(0)) == 60000


@pytest.mark.parametrize("filler", [
    'type: "xavier" sparse: 15', 'type: "constant" value: 1 sparse: 0',
    'type: "uniform" sparse: 3', 'type: "msra" sparse: 3',
    'type: "gaussian" sparse: 201', 'type: "gaussian" sparse: -2'])
def test_sparse_rejected(filler):
    ca.set_mode("cpu")
    with pytest.raises(ca.CaffeError, match="[Ss]pars"):
        ip_net(filler)


# initial weights of this net at seed 1234, recorded from the commit before
# `sparse` was read: without `sparse` no extra RNG draw may happen
RECORDED = {
    ("h", 0): [0.6195865869522095, 0.5601112842559814, -0.9692164063453674,
               0.14949798583984375, 0.31028687953948975,
               0.07139968872070312],
    ("h", 1): [0.25, 0.25],
    ("g", 0): [0.1025770753622055, -0.16809587180614471, 0.21814453601837158,
               -0.008744013495743275, 0.16902203857898712,
               -0.23841266334056854, 0.3118254244327545, -0.5592406988143921,
               0.30391162633895874, -0.1542321741580963, 0.11791523545980453,
               -0.3082348108291626],
    ("g", 1): [0.2567697763442993, -0.9608761072158813, -0.5864169597625732],
}


def test_weights_without_sparse_are_unchanged():
    ca.set_mode("cpu")
    ca.set_random_seed(1234)
    net = net_from_text("""name: "f"
layer { name: "in" type: "Input" top: "x" input_param { shape { dim: 2 dim: 4 } } }
layer { name: "g" type: "InnerProduct" bottom: "x" top: "g"
  inner_product_param { num_output: 3 weight_filler { type: "gaussian" std: 0.5 }
    bias_filler { type: "uniform" min: -1 max: 1 } } }
layer { name: "h" type: "InnerProduct" bottom: "g" top: "h"
  inner_product_param { num_output: 2 weight_filler { type: "xavier" }
    bias_filler { type: "constant" value: 0.25 } } }
""")
    seen = set()
    for i in range(net.num_params()):
        name, bidx, _ = net.param_info(i)
        seen.add((name, bidx))
        assert np.array_equal(net.param(i),
                              np.array(RECORDED[(name, bidx)], np.float32))
    assert seen == set(RECORDED)
