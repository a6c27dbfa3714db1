"""Input pipeline: oracle known-answer tests on CPU, GPU kernel vs oracle on the MI355X."""
import numpy as np
import pytest
import torch

import oracle


def test_resize_identity_and_ramp_known_answers():
    rs = np.random.RandomState(0)
    img = rs.uniform(-2, 2, (7, 9, 3)).astype(np.float32)
    assert np.array_equal(oracle.resize_linear_f32(img, (7, 9)), img)                     # same size: exact copy
    # 2x upsample of a horizontal ramp: half-pixel centres -> dst x maps to src (x+0.5)/2-0.5, clamped at the border
    ramp = np.tile(np.arange(4, dtype=np.float32)[None, :, None], (2, 1, 3))
    up = oracle.resize_linear_f32(ramp, (2, 8))[0, :, 0]
    np.testing.assert_allclose(up, [0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.0], atol=1e-6)
    # 2x downsample averages pixel pairs
    down = oracle.resize_linear_f32(ramp, (2, 2))[0, :, 0]
    np.testing.assert_allclose(down, [0.5, 2.5], atol=1e-6)
    # constant image stays constant under any resize
    c = np.full((5, 6, 3), 1.25, np.float32)
    assert np.allclose(oracle.resize_linear_f32(c, (11, 13)), 1.25)


@pytest.mark.parametrize("src,dst", [((375, 1242), (384, 1248)), ((370, 1224), (384, 1248)), ((50, 61), (64, 96)), ((123, 77), (64, 96)),
                                     ((800, 2000), (384, 1248)), ((9, 5), (17, 33))])
def test_resize_agrees_with_an_independent_half_pixel_bilinear(src, dst):
    """A second witness for the restated cv2.resize(INTER_LINEAR) (OpenCV itself is absent here: parity against cv2 stays unpinned):
    torch's ``F.interpolate(mode='bilinear', align_corners=False, antialias=False)`` implements the same published rule -- source
    coordinate (x + 0.5) * scale - 0.5, border clamp, no prefilter when shrinking -- independently of the oracle's code."""
    import torch.nn.functional as F
    rs = np.random.RandomState(3)
    img = rs.uniform(-2.5, 2.5, src + (3,)).astype(np.float32)
    # The witness runs in float64.  cv2 (and the oracle) round the source coordinate to float32 BEFORE splitting it into index and
    # weight, so at x ~ 1242 the weight is only good to one float32 ulp of the coordinate (1.2e-4 pixel); on this white-noise image
    # (neighbouring pixels differ by up to 5) that is up to ~6e-4 in the output.  A wrong rule (corner-aligned coordinates, a
    # missing half-pixel offset, a prefilter) would differ by O(1).
    want = F.interpolate(torch.from_numpy(img).double().permute(2, 0, 1)[None], size=dst, mode='bilinear', align_corners=False, antialias=False)
    want = want[0].permute(1, 2, 0).numpy()
    got = oracle.resize_linear_f32(img, dst)
    np.testing.assert_allclose(got, want, atol=6e-4, rtol=0)
    wrong = F.interpolate(torch.from_numpy(img).double().permute(2, 0, 1)[None], size=dst, mode='bilinear', align_corners=True)[0].permute(1, 2, 0).numpy()
    if src != dst:
        assert np.abs(got - wrong).max() > 0.05                           # (the comparison has teeth)


def test_preprocess_image_layout_and_scales():
    img = np.random.RandomState(1).randint(0, 256, (375, 1242, 3), dtype=np.uint8)
    x, scales = oracle.preprocess_image(img, (384, 1248))
    assert x.shape == (3, 384, 1248) and x.dtype == np.float32
    np.testing.assert_allclose(scales, [384 / 375., 1248 / 1242.], rtol=1e-7)
    # whitening statistics: channel c of a constant image
    const = np.zeros((10, 10, 3), np.uint8); const[:] = (93, 98, 95)
    y, _ = oracle.preprocess_image(const, (20, 20))
    exp = (np.array([93, 98, 95], np.float32) - oracle.KITTI_RGB_MEAN) / oracle.KITTI_RGB_STD
    np.testing.assert_allclose(y[:, 3, 4], exp, rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[(375, 1242), (370, 1224)], [(384, 1248)], [(50, 61), (123, 77), (9, 5)], [(800, 2000)]])
def test_gpu_preprocess_vs_oracle(sizes):
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    rs = np.random.RandomState(2)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    out, scales, meta = preprocess_batch(images, (384, 1248))
    assert tuple(out.shape) == (len(images), 3, 384, 1248)
    for b, im in enumerate(images):
        ref, sc = oracle.preprocess_image(im, (384, 1248))
        np.testing.assert_allclose(out[b].cpu().numpy(), ref, atol=2e-5, rtol=0)
        np.testing.assert_allclose(scales[b].cpu().numpy(), sc, rtol=1e-6)
        np.testing.assert_allclose(meta['scales'][b], sc, rtol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,target", [
    ([(33, 3001), (1, 1), (7, 1), (1, 9)], (384, 1248)),        # odd byte offsets, one-pixel sources, the packed buffer ends inside a dword
    ([(40, 3000), (3, 2731)], (64, 96)),                          # a row segment larger than the LDS staging buffer: direct path
    ([(40, 2728), (41, 2729)], (64, 96)),                         # ... and just inside it
    ([(375, 1242)] * 3, (384, 1248)),
    ([(97, 300), (13, 1023)], (61, 517)),                         # target not a multiple of the 4-row / 256-column workgroup tile
])
def test_gpu_preprocess_staged_rows_vs_oracle(sizes, target):
    """The resize kernel stages each workgroup's two source-row segments in LDS (aligned dwords; the tail of the packed buffer
    byte by byte) and whitens through a per-channel table: same values as the oracle's per-pixel arithmetic at every alignment."""
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    rs = np.random.RandomState(5)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    out, scales, _meta = preprocess_batch(images, target)
    for b, im in enumerate(images):
        ref, sc = oracle.preprocess_image(im, target)
        np.testing.assert_allclose(out[b].cpu().numpy(), ref, atol=2e-5, rtol=0)
        np.testing.assert_allclose(scales[b].cpu().numpy(), sc, rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,target", [
    ([(1, 1), (400, 1300), (383, 1249), (5, 2000), (390, 7)], (384, 1248)),
    ([(61, 517), (60, 516), (62, 519), (3, 3)], (61, 517)),
])
def test_gpu_padcrop_staged_rows_bit_exact_vs_oracle(sizes, target):
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    rs = np.random.RandomState(6)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    out, _shifts, meta = preprocess_batch(images, target, forbid_resize=True)
    for b, im in enumerate(images):
        ref, pad, crop = oracle.crop_or_pad_image(im, target, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD)
        assert np.array_equal(out[b].cpu().numpy(), ref), b
        assert meta['padding'][b].tolist() == list(pad) and meta['crops'][b].tolist() == list(crop)


@pytest.mark.gpu
def test_detect_images_end_to_end():
    """uint8 images -> GPU preprocess -> backbone -> fused detect, vs the oracle fed with the oracle's own
    pre-processed tensor (same kept anchors away from near-ties; boxes in original-image coordinates)."""
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    cfg = sqd.make_cfg()
    m = SqueezeDet(cfg); sd = synthetic.make_state_dict(); m.load_state_dict(sd)
    det = Detector(m, cfg)
    rs = np.random.RandomState(3)
    base = (rs.standard_normal((2, 48, 156, 3)) * 60 + 100)
    images = [np.clip(np.kron(base[0], np.ones((8, 8, 1))), 0, 255).astype(np.uint8)[:375, :1242],
              np.clip(np.kron(base[1], np.ones((8, 8, 1))), 0, 255).astype(np.uint8)[:370, :1224]]
    res = det.detect_images(images, image_ids=['a', 'b'])
    assert len(res) == 2
    for b, im in enumerate(images):
        x, sc = oracle.preprocess_image(im, cfg.input_size)
        with torch.no_grad():
            pred = oracle.backbone_forward(torch.from_numpy(x)[None], sd)
        ids, s, bx = oracle.inference_head(pred, cfg.anchors, cfg.input_size)
        d = oracle.filter_detections(ids[0].numpy(), s[0].numpy(), bx[0].numpy())
        r = res[b]
        assert r['image_meta']['image_id'] == ['a', 'b'][b]
        if d is None:
            assert 'boxes' not in r
            continue
        common = set(r['anchor_idx'].tolist()) & set(d['anchor_idx'].tolist())
        assert len(common) >= len(d['anchor_idx']) - 2
        ref_boxes = {int(i): bb for i, bb in zip(d['anchor_idx'], oracle.boxes_postprocess(d['boxes'], sc))}
        for i, bb in zip(r['anchor_idx'], r['boxes']):
            if int(i) in ref_boxes:
                np.testing.assert_allclose(bb, ref_boxes[int(i)], atol=2e-2)


class _FakeKitti:
    """The three members ``Detector.detect_dataset`` / ``DataWrapper`` use of the reference's dataset classes
    (src/datasets/kitti.py:47-55 ``load_image`` -> float32 RGB HWC + id; src/datasets/base.py:43-59 ``preprocess``)."""

    def __init__(self, images, input_size, integral=True):
        self.images, self.input_size, self.integral = images, input_size, integral

    def __len__(self):
        return len(self.images)

    def load_image(self, index):
        im = self.images[index].astype(np.float32)
        return (im if self.integral else im + 0.25), f'{index:06d}'

    def preprocess(self, image, image_meta, boxes=None):
        x = (image - oracle.KITTI_RGB_MEAN.reshape(1, 1, 3)) / oracle.KITTI_RGB_STD.reshape(1, 1, 3)
        scales = np.array([self.input_size[0] / image.shape[0], self.input_size[1] / image.shape[1]], dtype=np.float32)
        image_meta = dict(image_meta, scales=scales)
        return oracle.resize_linear_f32(x.astype(np.float32), self.input_size), image_meta, boxes


def test_data_wrapper_item_layout():
    from squeezedet_pytorch_amd.detector import DataWrapper
    rs = np.random.RandomState(5)
    ds = _FakeKitti([rs.randint(0, 256, (37, 53, 3), dtype=np.uint8), rs.randint(0, 256, (41, 60, 3), dtype=np.uint8)], (48, 64))
    w = DataWrapper(ds)
    assert len(w) == 2
    it = w[1]
    assert it['image'].shape == (3, 48, 64) and it['image'].dtype == np.float32
    m = it['image_meta']
    assert m['index'] == 1 and m['image_id'] == '000001' and m['orig_size'].tolist() == [41, 60, 3] and m['scales'].shape == (2,)


@pytest.mark.gpu
def test_detect_dataset_driver(capsys):
    """``Detector.detect_dataset`` (src/engine/detector.py:52-85): batches of raw images through the GPU input pipeline == calling
    ``detect_images`` batch by batch (ragged last batch, dataset indices in ``image_meta``), the reference's two kinds of log
    lines, the empty dataset; a dataset whose pixels are not uint8-representable takes the host route (``dataset.preprocess`` +
    ``detect``) and agrees with the GPU route up to the pre-processing difference of a quarter grey level."""
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    cfg = sqd.make_cfg()
    cfg.batch_size, cfg.num_workers, cfg.print_interval = 2, 2, 1
    m = SqueezeDet(cfg); m.load_state_dict(synthetic.make_state_dict())
    det = Detector(m, cfg)
    rs = np.random.RandomState(3)
    base = rs.standard_normal((5, 48, 156, 3)) * 60 + 100
    sizes = [(375, 1242), (370, 1224), (375, 1242), (374, 1238), (376, 1241)]
    images = [np.clip(np.kron(base[i], np.ones((8, 8, 1))), 0, 255).astype(np.uint8)[:h, :w] for i, (h, w) in enumerate(sizes)]
    ds = _FakeKitti(images, cfg.input_size)
    res = det.detect_dataset(ds)
    out = capsys.readouterr().out
    assert out.count('eval: [') == 3 and 'Elapsed' in out and 'frames/s' in out
    assert len(res) == 5 and [r['image_meta']['index'] for r in res] == [0, 1, 2, 3, 4]
    assert [r['image_meta']['image_id'] for r in res] == [f'{i:06d}' for i in range(5)]
    want = det.detect_images(images[0:2]) + det.detect_images(images[2:4]) + det.detect_images(images[4:5])
    assert sum('boxes' in r for r in want) >= 3
    for r, w in zip(res, want):
        assert ('boxes' in r) == ('boxes' in w)
        if 'boxes' in r:
            assert np.array_equal(r['anchor_idx'], w['anchor_idx']) and np.array_equal(r['boxes'], w['boxes']) and np.array_equal(r['scores'], w['scores'])
        assert r['image_meta']['orig_size'].tolist() == w['image_meta']['orig_size'].tolist()
    assert det.detect_dataset(_FakeKitti([], cfg.input_size)) == []
    # host route: pixels + 0.25 are not uint8-representable
    res_h = det.detect_dataset(_FakeKitti(images, cfg.input_size, integral=False))
    assert len(res_h) == 5 and [r['image_meta']['index'] for r in res_h] == [0, 1, 2, 3, 4]
    for r, w in zip(res_h, want):
        if 'boxes' in r and 'boxes' in w:
            common = set(r['anchor_idx'].tolist()) & set(w['anchor_idx'].tolist())
            assert len(common) >= min(len(r['anchor_idx']), len(w['anchor_idx'])) - 3


_GEOMETRY_STEM = {'resize': 'sqd_preprocess_u8', 'padcrop': 'sqd_preprocess_u8_padcrop', 'letterbox': 'sqd_preprocess_u8_letterbox'}
_FORMS = [(False, False, '_fwd'), (True, False, '_aug_fwd'), (True, True, '_aug_color_fwd')]


@pytest.mark.parametrize("geometry", list(_GEOMETRY_STEM))
@pytest.mark.parametrize("aug,color,suffix", _FORMS)
def test_launch_u8_selects_the_entry_and_assembles_its_arguments(geometry, aug, color, suffix):
    """The one Python dispatch against ``_native._SIGNATURES``, without a launch: every argument a non-null host address that is never
    dereferenced and ``B = 0``, so the entry that was selected answers status 1 itself -- a wrong argument count or type would be a ctypes
    error instead, and the message names the entry that was called."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from squeezedet_pytorch_amd import _native as nat
    from squeezedet_pytorch_amd import preprocess as pre
    want = _GEOMETRY_STEM[geometry] + suffix
    assert pre.entry_name(geometry, aug, color) == want and want in nat._SIGNATURES
    keep = (ctypes.c_ulonglong * 8)()
    p = ctypes.c_void_p(ctypes.addressof(keep))
    blocks = {'resize': dict(scales=p), 'padcrop': dict(shifts=p, padcrop=p), 'letterbox': dict(win=p, scales=p, shifts=p)}[geometry]
    if aug:
        blocks.update(aug=p)
    if color:
        blocks.update(color=p, sums=p)
    with pytest.raises(RuntimeError) as e:
        pre.launch_u8(geometry, p, p, p, p, 0, 8, 8, (1., 2., 3.), (4., 5., 6.), None, stream=ctypes.c_void_p(0), **blocks)
    assert str(e.value) == f'{want}: bad argument (status 1)'
    # the optional outputs may be left out (NULL)
    with pytest.raises(RuntimeError, match=want + ': bad argument'):
        pre.launch_u8(geometry, p, p, p, p, 0, 8, 8, (1., 2., 3.), (4., 5., 6.), None, stream=ctypes.c_void_p(0),
                      **{k: v for k, v in blocks.items() if k in ('aug', 'color', 'sums')})


def test_launch_u8_refuses_combinations_without_an_entry():
    import ctypes
    from squeezedet_pytorch_amd import preprocess as pre
    keep = (ctypes.c_ulonglong * 8)()
    p = ctypes.c_void_p(ctypes.addressof(keep))

    def call(geometry, **blocks):
        pre.launch_u8(geometry, p, p, p, p, 0, 8, 8, (1., 2., 3.), (4., 5., 6.), None, stream=ctypes.c_void_p(0), **blocks)

    for geometry in _GEOMETRY_STEM:
        with pytest.raises(ValueError):
            call(geometry, color=p, sums=p)                              # colour without aug
        with pytest.raises(ValueError):
            call(geometry, aug=p, color=p)                               # colour without the channel sums
    for geometry in ('resize', 'padcrop'):
        with pytest.raises(ValueError):
            call(geometry, win=p)                                        # a window outside letterbox
        with pytest.raises(ValueError):
            call(geometry, aug=p, win=p)
    with pytest.raises(ValueError):
        call('letterbox', padcrop=p)                                     # letterbox with pad / crop outputs
    with pytest.raises(ValueError):
        call('resize', padcrop=p)
    with pytest.raises(ValueError):
        call('resize', shifts=p)
    with pytest.raises(ValueError):
        call('padcrop', scales=p)
    with pytest.raises(ValueError):
        call('stretch')
    with pytest.raises(ValueError):
        pre.entry_name('resize', aug=False, color=True)


def test_pad_crop_equals_the_three_formulas_it_replaces():
    """``boxes.pad_crop`` against the three earlier spellings of crop_or_pad's integers (image.py:99-115), each restated here as it stood:
    the [B, 4] array loop of ``preprocess_batch``, the per-image array loop of ``DetectStream._image_meta`` and the tuple of
    ``augment._pad_crop``; every (size, target) in 1..40 squared, size == target included."""
    from squeezedet_pytorch_amd.boxes import pad_crop

    def batch_form(size, target):
        padding, crops = np.zeros((1, 4), np.int16), np.zeros((1, 4), np.int16)
        for s, t, k in ((size, target, 0),):
            if s < t:
                padding[0, k] = (t - s) // 2; padding[0, k + 1] = (t - s) - padding[0, k]
            elif s > t:
                crops[0, k] = (s - t) // 2; crops[0, k + 1] = (s - t) - crops[0, k]
        return int(padding[0, 0]), int(padding[0, 1]), int(crops[0, 0]), int(crops[0, 1])

    def stream_form(size, target):
        pad, crop = np.zeros(4, np.int16), np.zeros(4, np.int16)
        for s, t, k in ((int(size), target, 2),):
            if s < t:
                pad[k] = (t - s) // 2; pad[k + 1] = (t - s) - pad[k]
            elif s > t:
                crop[k] = (s - t) // 2; crop[k + 1] = (s - t) - crop[k]
        return int(pad[2]), int(pad[3]), int(crop[2]), int(crop[3])

    def tuple_form(size, target):
        if size < target:
            return (target - size) // 2, (target - size) - (target - size) // 2, 0, 0
        if size > target:
            return 0, 0, (size - target) // 2, (size - target) - (size - target) // 2
        return 0, 0, 0, 0

    for size in range(1, 41):
        for target in range(1, 41):
            got = pad_crop(size, target)
            assert all(isinstance(v, int) for v in got)
            assert got == batch_form(size, target) == stream_form(size, target) == tuple_form(size, target), (size, target)
            assert got[0] + got[1] + size - got[2] - got[3] == target
