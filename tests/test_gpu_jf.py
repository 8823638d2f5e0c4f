"""GPU tests of the J&F counts kernel (fgvc_jf_counts_u8) and of the paths that use it: the counts against the
numpy restatement of tests/jf_cases.py with `==` on every case, metrics' backend='hip' against the host scorer with `==`, the trackers'
test_cfg.masks='device', and datasets.davis_evaluate.  J and F are ratios of integer counts: there is no tolerance here but the golden
file's own 1e-12."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import jf_cases as JC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(JC.cases())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _want(name):
    return torch.from_numpy(JC.expected(name))


def _report(name, got, want):
    bad = (got != want).nonzero()
    return f"{name}: {bad.shape[0]} counts differ; first (frame, object, count) {bad[:4].tolist()}: got {got[tuple(bad[0])] if len(bad) else ''}, " \
           f"want {want[tuple(bad[0])] if len(bad) else ''}"


@pytest.mark.parametrize("name", NAMES)
def test_counts_equal_the_restatement(dev, name):
    from fgvc_amd import ops
    gt, pred, n, r = JC.cases()[name]
    got = ops.jf_counts(torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev), n, r)
    assert got.dtype == torch.int64 and tuple(got.shape) == (gt.shape[0], n, 6)
    assert torch.equal(got.cpu(), _want(name)), _report(name, got.cpu(), _want(name))


@pytest.mark.parametrize("name", ["two_words_plus_one_3x33x129", "blobs_2x48x64"])
def test_out_side_stream_and_sliced_view(dev, name):
    from fgvc_amd import ops
    gt, pred, n, r = JC.cases()[name]
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    want = _want(name)
    out = torch.full((gt.shape[0], n, 6), -7, device=dev, dtype=torch.int64)            # every element is written: nothing to clear
    assert ops.jf_counts(g, p, n, r, out=out) is out and torch.equal(out.cpu(), want)
    assert torch.equal(ops.jf_counts(g, p, n, r, out=out).cpu(), want)                  # a second call on the same buffer
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = ops.jf_counts(g, p, n, r)
    side.synchronize()
    assert torch.equal(got.cpu(), want)
    # non-contiguous frame views: every other frame of an interleaved stack, and a cropped window
    g2, p2 = torch.stack([g, p], 1).reshape(-1, *g.shape[1:]), torch.stack([p, g], 1).reshape(-1, *g.shape[1:])
    assert not g2[::2].is_contiguous() or g.shape[0] == 1
    assert torch.equal(ops.jf_counts(g2[::2], p2[::2], n, r).cpu(), want)
    big_g, big_p = torch.full((g.shape[0], g.shape[1] + 3, g.shape[2] + 5), 1, device=dev, dtype=torch.uint8), \
        torch.full((g.shape[0], g.shape[1] + 3, g.shape[2] + 5), 2, device=dev, dtype=torch.uint8)
    big_g[:, 2:-1, 4:-1], big_p[:, 2:-1, 4:-1] = g, p
    assert torch.equal(ops.jf_counts(big_g[:, 2:-1, 4:-1], big_p[:, 2:-1, 4:-1], n, r).cpu(), want)
    with pytest.raises(ValueError, match="out"):
        ops.jf_counts(g, p, n, r, out=torch.empty((gt.shape[0], n, 6), device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="out"):
        ops.jf_counts(g, p, n, r, out=torch.empty((gt.shape[0], n + 1, 6), device=dev, dtype=torch.int64))
    with pytest.raises(TypeError, match="uint8"):
        ops.jf_counts(g.float(), p, n, r)
    with pytest.raises(ValueError, match="radius"):
        ops.jf_counts(g, p, n, 65)
    assert tuple(ops.jf_counts(g, p, 0, r).shape) == (gt.shape[0], 0, 6) and tuple(ops.jf_counts(g[:0], p[:0], n, r).shape) == (0, n, 6)


def test_jfm_on_the_golden_masks(dev):
    from fgvc_amd import metrics
    g = np.load(os.path.join(ROOT, "tests", "golden", "vos_jf.npz"))
    gt, pr = g["gt"], g["pred"]
    host, hip = metrics.JFM(gt, pr, gt.shape[0]), metrics.JFM(gt, pr, gt.shape[0], backend="hip")
    assert hip == host
    for k in ("JM", "JR", "JD", "FM", "FR", "FD"):
        np.testing.assert_allclose(np.asarray(hip[k]), g["JFM_" + k], rtol=0, atol=1e-12)
    assert hip == metrics.JFM(torch.from_numpy(gt).to(dev), torch.from_numpy(pr).to(dev), backend="hip")
    assert metrics.JFM(gt, pr[:2], backend="hip") == metrics.JFM(gt, pr[:2])             # a missing object: padded with an empty mask
    for o in range(gt.shape[0]):
        assert np.array_equal(metrics.db_eval_boundary(gt[o], pr[o], backend="hip"), metrics.db_eval_boundary(gt[o], pr[o]))
    assert metrics.db_eval_boundary(gt[0, 3], pr[0, 3], backend="hip") == metrics.db_eval_boundary(gt[0, 3], pr[0, 3])


def test_davis_jf_hip_equals_host(dev):
    from fgvc_amd import metrics
    s = JC.davis_sequences()
    assert s["two"][0].shape[0] == 2 and s["six"][0].shape[0] == 6
    host = metrics.davis_jf(s)
    assert metrics.davis_jf(s, backend="hip") == host                                    # float64 numpy predictions
    on_dev = {k: (gt, torch.from_numpy(pred.astype(np.uint8)).to(dev)) for k, (gt, pred) in s.items()}
    assert metrics.davis_jf(on_dev, backend="hip") == host                               # uint8 CUDA predictions, in place
    both = {k: (torch.from_numpy(gt).to(dev), p) for k, (gt, p) in on_dev.items()}
    assert metrics.davis_jf(both, backend="hip") == host
    # a prediction with an id the annotation does not have, and a fractional one: rint, then no object
    gt, pred = s["six"]
    odd = pred.copy()
    odd[2, :5, :5], odd[3, 10:14, 10:14] = 9.0, 1.4
    assert metrics.davis_jf({"odd": (gt, odd)}, backend="hip") == metrics.davis_jf({"odd": (gt, odd)})
    with pytest.raises(TypeError, match="uint8"):
        metrics.davis_jf({"f": (gt, torch.from_numpy(pred).to(dev))}, backend="hip")


@pytest.mark.parametrize("typ", ["VanillaTracker", "HRVanillaTracker"])
def test_masks_device_is_the_same_masks(dev, typ):
    """The tiny clip of tests/test_gpu_vos.py's key test: test_cfg.masks='device' returns the uint8 tensor the default call converts."""
    import fgvc_amd.mmpt_api as api

    def model(**extra):
        cfg = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True, with_first_neighbor=True, **extra)
        torch.manual_seed(0)
        m = api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                            test_cfg=cfg)
        m.init_weights()
        return m.to(dev).eval()
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(1, 1, 3, 5, 40, 44, generator=g).to(dev)
    seg = torch.zeros(1, 40, 44, dtype=torch.long)
    seg[0, 5:20, 5:20], seg[0, 22:38, 20:40] = 1, 2
    call = dict(test_mode=True, imgs=imgs, ref_seg_map=seg.to(dev), img_meta=[dict(original_shape=(40, 44))])
    host = model()(**call)
    on_dev = model(masks="device")(**call)
    assert isinstance(host[0], np.ndarray) and host[0].dtype == np.float64
    assert isinstance(on_dev, list) and len(on_dev) == 1
    m = on_dev[0]
    assert isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape) == (5, 40, 44)
    assert np.array_equal(m.cpu().numpy().astype(np.float64), host[0])
    assert np.array_equal(model(masks="numpy")(**call)[0], host[0])


def test_davis_evaluate_hip_equals_host(dev, tmp_path):
    import fgvc_amd.mmpt_api as api
    from fgvc_amd.datasets import Davis2017, davis_evaluate
    spec = importlib.util.spec_from_file_location("make_fake_davis", os.path.join(ROOT, "tools", "make_fake_davis.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    mk.make(str(tmp_path), sequences=2, frames=6, size=(61, 75), objects=3, seed=1)
    ds = Davis2017(str(tmp_path), device=dev)

    def model(**extra):
        cfg = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True, with_first_neighbor=True, **extra)
        torch.manual_seed(0)
        m = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                       pool_type="none")), test_cfg=cfg)
        m.init_weights()
        return m.to(dev).eval()
    host = davis_evaluate(model(), ds)
    assert davis_evaluate(model(masks="device"), ds, backend="hip") == host              # masks stay on the device
    assert davis_evaluate(model(), ds, backend="hip") == host                            # float64 host masks, uploaded
    assert 0.0 <= host["J&F-Mean"] <= 1.0
