"""GPU tests of the box stage of the renderer (fgvc_render_boxes_u8): backend='hip' against backend='host' with `==` on
every case of tests/objects_cases.py (frames of 3 x 37 x 300: two column tiles, five row bands), in place, on strided frames, on device
tensors, and the refusals by name.  The arithmetic is integer: there is no tolerance."""
import numpy as np
import pytest
import torch

from tests import objects_cases as OC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _report(name, got, want):
    bad = np.argwhere(got != want)
    return f"{name}: {len(bad)} bytes differ; first (frame, y, x, channel) {bad[:4].tolist()}"


@pytest.mark.parametrize("name", list(OC.box_cases()))
def test_hip_equals_host(dev, name):
    from fgvc_amd import viz
    kw = OC.box_cases()[name]
    want = OC.box_expected(name)
    got = viz.render(backend="hip", **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), _report(name, got, want)
    if name not in ("no_box",):
        assert not np.array_equal(want, viz.render(**{k: v for k, v in kw.items() if not k.startswith(("box", "label"))}))   # the boxes drew something


def test_tile_is_the_one_the_cases_assume(dev):
    from fgvc_amd import ops
    assert ops.RENDER_TILE == (8, 256)


def test_in_place_strided_and_device_tensors(dev):
    from fgvc_amd import ops, viz
    kw = OC.box_cases()["with_overlay_and_dots"]
    want = torch.from_numpy(np.array(OC.box_expected("with_overlay_and_dots")))
    f = torch.from_numpy(np.array(kw["frames"])).to(dev)
    args = dict(ids=torch.from_numpy(np.array(kw["ids"])).to(dev), tracks=torch.from_numpy(kw["tracks"].copy()).to(dev), radius=kw["radius"])
    boxes = torch.from_numpy(np.array(kw["boxes"])).to(dev)
    labels = torch.tensor(kw["box_labels"], device=dev)
    # device tensors through viz.render: a device tensor comes back
    got = viz.render(f, backend="hip", boxes=boxes, box_labels=labels, **args)
    assert got.is_cuda and torch.equal(got.cpu(), want)
    # in place
    g = f.clone()
    assert ops.render_boxes(g, boxes, box_labels=labels, out=g, **args) is g and torch.equal(g.cpu(), want)
    # strided frames and a strided `out`: a window of a larger video and every second frame of a longer one
    big = torch.zeros((OC.BOX_T, OC.BOX_H + 3, OC.BOX_W + 5, 3), dtype=torch.uint8, device=dev)
    big[:, 1:-2, 2:-3] = f
    got = ops.render_boxes(big[:, 1:-2, 2:-3], boxes, box_labels=labels, **args)
    assert torch.equal(got.cpu(), want)
    long = f.repeat_interleave(2, 0)
    out = torch.zeros_like(long)
    ops.render_boxes(long[::2], boxes, box_labels=labels, out=out[::2], **args)
    assert torch.equal(out[::2].cpu(), want) and int(out[1::2].max()) == 0


def test_refusals_by_name(dev):
    from fgvc_amd import ops, viz
    f = OC.box_frames()
    b = np.array([[[1, 1, 5, 5]]] * OC.BOX_T)
    tr = np.zeros((1, OC.BOX_T, 2))
    with pytest.raises(ValueError, match="trail"):
        viz.render(f, tracks=tr, trail=2, boxes=b, backend="hip")
    with pytest.raises(ValueError, match="skeleton"):
        viz.render(f, tracks=tr, skeleton=[[0, 0]], boxes=b, backend="hip")
    with pytest.raises(ValueError, match="heat"):
        viz.render(f, heat=np.zeros((OC.BOX_T, 1, OC.BOX_H, OC.BOX_W), np.float32), boxes=b, backend="hip")
    with pytest.raises(ValueError, match="boxes: N=256"):
        viz.render(f, boxes=np.zeros((OC.BOX_T, 256, 4), np.int64), backend="hip")
    with pytest.raises(ValueError, match=r"boxes: coordinates below 2\*\*20"):
        viz.render(f, boxes=np.array([[[0, 0, 2 ** 20, 5]]] * OC.BOX_T), backend="hip")
    d = torch.from_numpy(f).to(dev)
    with pytest.raises(ValueError, match=r"boxes: coordinates below 2\*\*20"):
        ops.render_boxes(d, torch.tensor([[[0, -2 ** 20, 4, 5]]] * OC.BOX_T, device=dev))
    with pytest.raises(ValueError, match="box_width"):
        ops.render_boxes(d, torch.from_numpy(b).to(dev), box_width=17)
    with pytest.raises(ValueError, match="box_alpha"):
        ops.render_boxes(d, torch.from_numpy(b).to(dev), box_alpha=257)
    with pytest.raises(ValueError, match="label_scale"):
        ops.render_boxes(d, torch.from_numpy(b).to(dev), label_scale=5)
    with pytest.raises(ValueError, match="box_labels"):
        ops.render_boxes(d, torch.from_numpy(b).to(dev), box_labels=torch.tensor([1000], device=dev))
    with pytest.raises(ValueError, match="box_visibles"):
        ops.render_boxes(d, torch.from_numpy(b).to(dev), box_visibles=torch.ones((OC.BOX_T, 2), dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="box_colors"):
        ops.render_boxes(d, torch.from_numpy(b).to(dev), box_colors=torch.zeros((2, 3), dtype=torch.uint8, device=dev))
