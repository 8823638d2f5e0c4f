"""The stride-2 block's 1x1 / stride 2 projection riding in the launch of its 3x3 / stride 2 convolution
(fgvc_conv_s2_split_proj_fmt_f32, conv_s2_kernel<3, true>): every output equals the two separate launches BIT FOR BIT -- the
projection's pixels are the 3x3 kernel's centre tap and every sum keeps its order -- in the kernel alone and through the trunk
(ResNet.fuse_s2_projection).  The refusals of the wrapper and of the C entry, and the kernel's register count, are checked on the host."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _bn(C, g):
    bn = torch.nn.BatchNorm2d(C).eval()
    bn.weight.data = torch.rand(C, generator=g) + 0.5
    bn.bias.data = torch.randn(C, generator=g) * 0.3          # (a projection bias != 0)
    bn.running_mean = torch.randn(C, generator=g) * 0.1
    bn.running_var = torch.rand(C, generator=g) + 0.5
    return bn


def _operands(N, H, W, Cin, Cout, dev, seed):
    """seeded input in the split form the kernels read, and both weight sets in their operand order"""
    from fgvc_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w3 = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5
    w1 = torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cin) ** 0.5
    c3 = ops.prepare_conv_s2(w3.to(dev), _bn(Cout, g).to(dev))
    c1 = ops.prepare_conv_s2(w1.to(dev), _bn(Cout, g).to(dev))
    return ops.nchw_to_split_nhwc(x.to(dev)), c3, c1


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _both_routes(xs, c3, c1, N, H, W, Cout, dev, relu, relu2, fmt, so, want_f32):
    """(split, f32 or None, projection, overflow word) of the two launches and of the fused one"""
    from fgvc_amd import ops
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    res = []
    for fused in (False, True):
        s = ops.alloc_split_nhwc(N, Cout, Ho, Wo, dev)
        f = torch.full((N, Ho, Wo, Cout), float("nan"), device=dev) if want_f32 else None
        pj = torch.full((N, Ho, Wo, Cout), float("nan"), device=dev)
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dict(out_split=s, out_f32=f, out_fmt=fmt, out_scale_log2=so, overflow=ovf)
        if fused:
            ops.conv_s2_split(xs, c3[0], c3[1], H, W, relu, proj=(c1[0], c1[1], pj), proj_relu=relu2, **kw)
        else:
            ops.conv_s2_split(xs, c1[0], c1[1], H, W, relu2, out_f32=pj)
            ops.conv_s2_split(xs, c3[0], c3[1], H, W, relu, **kw)
        res.append((s, f, pj, int(ovf.item())))
    return res


def _scale_log2(xs, c3, N, H, W, Cout, dev):
    """the f16 scale the encoder would calibrate for the 3x3 output (largest value into (2^7, 2^8])"""
    from fgvc_amd import ops
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    f = ops.alloc_nhwc(N, Cout, Ho, Wo, dev)
    ops.conv_s2_split(xs, c3[0], c3[1], H, W, True, out_f32=f)
    return ops.act_scale_log2(float(f.abs().max()))


# (N, H, W of the input), Cin, Cout, raise the overflow word
SHAPES = [((1, 7, 9), 64, 128, False),        # one partial tile; odd sizes: the last row and column come from the border
          ((2, 9, 67), 64, 128, True),        # two tile columns, the second with 2 valid pixels; batch index in the addresses
          ((1, 18, 130), 64, 128, False),     # tile rows 4 + 4 + 1; three tile columns
          ((1, 10, 66), 128, 256, False)]     # four chunks; two output-channel groups (blockIdx.y)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_launch_equals_the_two_launches(dev, shape):
    """3x3 split output (whole padded tensor: the zero border too) in the bf16 and the f16 + FP6 form, its dense f32 output where
    asked for, the projection's f32 output and the overflow word: equal bits; one case scaled so that the word is raised."""
    from fgvc_amd import ops
    (N, H, W), Cin, Cout, raise_ovf = shape
    xs, c3, c1 = _operands(N, H, W, Cin, Cout, dev, 11 + N + H + W + Cin)
    so = _scale_log2(xs, c3, N, H, W, Cout, dev)
    forms = [(ops.ACT_BF16X2, 0, 0), (ops.ACT_F16F6, so, 0)] + ([(ops.ACT_F16F6, so + 9, 1)] if raise_ovf else [])   # 2^17 times the largest value
    for fmt, scale, want_word in forms:
        for want_f32 in (False, True):
            (s0, f0, p0, o0), (s1, f1, p1, o1) = _both_routes(xs, c3, c1, N, H, W, Cout, dev, True, False, fmt, scale, want_f32)
            what = (shape, fmt, scale, want_f32)
            assert torch.equal(s0, s1), what
            assert not want_f32 or torch.equal(_bits(f0), _bits(f1)), what
            assert torch.equal(_bits(p0), _bits(p1)), what
            assert o0 == o1 == want_word, (what, o0, o1)
            assert bool(torch.isfinite(p1).all()) and (not want_f32 or bool(torch.isfinite(f1).all())), what      # every pixel was written
            assert int(s1.view(torch.int16).abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("relu2", [False, True])
def test_flags_do_not_cross_between_the_two_paths(dev, relu, relu2):
    """each path keeps its own ReLU flag and its own bias (the projection's is not zero)"""
    from fgvc_amd import ops
    N, H, W, Cin, Cout = 1, 8, 64, 64, 128
    xs, c3, c1 = _operands(N, H, W, Cin, Cout, dev, 5)
    assert float(c1[1].abs().min()) > 0 and not torch.equal(c1[1], c3[1])
    (s0, f0, p0, _), (s1, f1, p1, _) = _both_routes(xs, c3, c1, N, H, W, Cout, dev, relu, relu2, ops.ACT_BF16X2, 0, True)
    assert torch.equal(s0, s1) and torch.equal(_bits(f0), _bits(f1)) and torch.equal(_bits(p0), _bits(p1))
    assert bool((f1 < 0).any()) == (not relu) and bool((p1 < 0).any()) == (not relu2)


@pytest.mark.gpu
def test_trunk_with_and_without_the_fused_launch(dev, monkeypatch):
    """ResNet.fuse_s2_projection on / off: the same stage outputs bit for bit, on the route whose last convolution writes the feature
    bank and on the dense one; with the switch on the stride-2 block is ONE launch (calibration passes aside), off it is two."""
    import fgvc_amd.mmpt_api as api
    from fgvc_amd import ops
    from fgvc_amd.mmpt_api.backbones import ResNet
    from oracle import fgvc_oracle as O
    calls = []
    real = ops.conv_s2_split
    monkeypatch.setattr(ops, "conv_s2_split", lambda *a, **k: (calls.append(k.get("proj") is not None), real(*a, **k))[1])
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(21)).to(dev)
    yes = lambda C, H, W: True
    assert ResNet.fuse_s2_projection
    for out_indices in ((2,), (1, 2)):
        net = api.build_backbone(dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=out_indices, pool_type="none"))
        net.load_state_dict(O.seeded_resnet_state(3, (1, 2, 1, 1), "none"))
        net = net.to(dev).eval()
        if len(out_indices) == 1:
            routes = [lambda: [net.forward_hwc(x, True, split_if=yes, split_fmt="f16f6x")[0].clone()],      # banked
                      lambda: [net.forward_hwc(x, True)[0].clone()]]                                        # dense rows
        else:
            routes = [lambda: [t.clone() for t in net(x)]]                                                  # stage outputs, NCHW
        with torch.no_grad():
            for run in routes:
                run()                                                  # (calibrates: two launches whatever the switch says)
                del calls[:]
                on = run()
                assert calls and all(calls), calls                     # every stride-2 block in one launch
                try:
                    ResNet.fuse_s2_projection = False
                    del calls[:]
                    off = run()
                    assert calls and not any(calls) and len(calls) % 2 == 0, calls
                finally:
                    ResNet.fuse_s2_projection = True
                assert len(on) == len(off) == len(out_indices)
                for a, b in zip(on, off):
                    assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))
        assert not net.check_overflow()


def test_fused_kernel_keeps_two_workgroups_per_cu():
    """what the compiler allocated for conv_s2_kernel<3, true>, from the code-object notes of the built library (no GPU): at most 128
    registers -- four waves per SIMD, i.e. two 512-thread workgroups per CU, as for the plain 3x3 kernel -- and no scratch."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_notes", os.path.join(root, "tools", "kernel_notes.py"))
    kn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kn)
    notes = kn.kernel_notes()
    for inst in ("conv_s2_kernelILi3ELb1E", "conv_s2_kernelILi3ELb0E", "conv_s2_kernelILi1ELb0E"):
        ks = {k: v for k, v in notes.items() if inst in k}
        assert len(ks) == 1, (inst, sorted(notes)[:5])
        for k, v in ks.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 128, (k, v)


def test_projection_arguments_are_refused_on_the_host():
    """mismatched Cout, a projection beside the 1x1 form, wrong weight shapes: the wrapper raises before anything touches a device
    (CPU tensors here), the C entry answers FGVC_ERR_UNSUPPORTED / FGVC_ERR_INVALID_ARG before any launch."""
    from fgvc_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    N, H, W, Cin = 1, 8, 8, 64
    prep = lambda Cout, KS: ops.prepare_conv_s2(torch.randn(Cout, Cin, KS, KS, generator=g), _bn(Cout, g))
    c3, c1, c1_wide, c3_too = prep(128, 3), prep(128, 1), prep(256, 1), prep(128, 3)
    Hp, Wp = ops.conv_pad_dims(H, W)
    xs = torch.zeros(N, Hp, Wp, Cin // 32, 64, dtype=torch.int16)
    out = lambda C: torch.zeros(N, 4, 4, C)
    call = lambda w, pj: ops.conv_s2_split(xs, w[0], w[1], H, W, True, out_f32=out(128), proj=pj)
    with pytest.raises(ValueError, match="Cout"):
        call(c3, (c1_wide[0], c1_wide[1], out(256)))
    with pytest.raises(ValueError, match="Cout"):
        call(c3, (c1[0], c1_wide[1], out(128)))
    with pytest.raises(ValueError, match="3x3"):
        call(c1, (c1[0], c1[1], out(128)))
    with pytest.raises(ValueError, match="1x1 form"):
        call(c3, (c3_too[0], c3_too[1], out(128)))                    # nine taps where the projection's one belongs
    with pytest.raises(ValueError, match="1x1 form"):
        call(c3, (c1[0][:, :1], c1[1], out(128)))                     # one chunk of two
    with pytest.raises(ValueError, match="1x1 form"):
        call(c3, (c1[0].reshape(1, 2, 4, 64, 4, 8), c1[1], out(128)))
    with pytest.raises(ValueError, match="output"):
        call(c3, (c1[0], c1[1], torch.zeros(N, 4, 5, 128)))
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        call(c3, (c1[0], c1[1], out(128)))                            # well-formed: only the device is wrong
    # the C entry (pointers are never followed: every refusal comes before the launch)
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p = lambda i: ctypes.c_void_p(base + 256 * i)
    Hop, Wop = ops.conv_pad_dims(4, 4)
    entry = lambda KS, Cout2, w2=p(5), b2=p(6), y2=p(7): lib.fgvc_conv_s2_split_proj_fmt_f32(
        p(0), p(1), p(2), p(3), p(4), w2, b2, y2, N, H, W, Hp, Wp, Cin, 128, KS, Cout2, Hop, Wop, 1, 0, 0, 0, None, None)
    assert entry(1, 128) == _lib.ERR_UNSUPPORTED and b"3x3" in lib.fgvc_last_error()
    assert entry(3, 256) == _lib.ERR_UNSUPPORTED and b"Cout" in lib.fgvc_last_error()
    assert entry(3, 128, b2=None) == _lib.ERR_INVALID_ARG and b"go together" in lib.fgvc_last_error()
    assert entry(3, 128, y2=p(4)) == _lib.ERR_INVALID_ARG and b"differ" in lib.fgvc_last_error()
