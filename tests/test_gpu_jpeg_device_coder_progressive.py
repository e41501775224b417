"""GPU parity of the device entropy coder's optimised-table and progressive forms (csrc/jpeg_encode_progressive.hip,
ifhip_jpeg_encode_flags_batch_device): the files it leaves in HBM are byte-identical to libjpeg-turbo's (Pillow wrote the
file; the coefficients come from its baseline twin through the oracle's entropy decoder) and to the host writer's."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import oracle as O
from imageflow_amd.codecs import mozjpeg as M
from imageflow_amd.graphics.bitmaps import Bitmap
from tests.test_jpeg_device_coder import SAMPLINGS, photo
from tests.test_jpeg_device_coder_progressive import FLAGS, flat_gray, host_writer, noise_gray, save, synthetic_planes, twin
from tests.test_gpu_jpeg_device_coder import coder_for, planes_of

pytestmark = pytest.mark.gpu


def kw(flags):
    return {"progressive": bool(flags & 2), "optimize_coding": bool(flags & 1)}


@pytest.mark.parametrize("sampling", ["4:2:0", "4:2:2", "4:4:4"])
@pytest.mark.parametrize("size", [(1, 1), (17, 9), (64, 48), (203, 131), (640, 360)])
def test_files_equal_libjpeg_turbos(sampling, size):
    w, h = size
    coder = None
    for q in (5, 75, 90, 100):
        img = photo(w, h, w * 31 + h + q)
        j = twin(img, q, sampling)
        assert (j["hs"], j["vs"]) == SAMPLINGS[sampling]
        coder = coder or coder_for(j, 1)
        planes = planes_of([j])
        for flags in (1, 2, 3):
            files, status = coder.encode(planes, q, **kw(flags))
            assert status == [0], (q, flags)
            assert files[0] == save(img, q, sampling, **FLAGS[flags]), (q, flags)


def test_grayscale():
    img = photo(150, 97, 3)[:, :, 0]
    j = twin(img, 80)
    coder = coder_for(j, 1)
    for flags in (1, 2, 3):
        assert coder.encode(planes_of([j]), 80, **kw(flags)) == ([save(img, 80, **FLAGS[flags])], [0])


def test_flat_frame_one_run_of_33124_blocks():
    img = flat_gray()
    j = twin(img, 75)
    assert coder_for(j, 1).encode(planes_of([j]), 75, progressive=True) == ([save(img, 75, progressive=True)], [0])


def test_noise_at_q100_correction_bit_cuts_and_stuffing():
    img = noise_gray()
    j = twin(img, 100)
    data = save(img, 100, progressive=True)
    assert data.count(b"\xff\x00") > 100
    coder = coder_for(j, 1)
    assert len(data) <= coder.max_file_bytes_for(progressive=True)
    assert coder.max_file_bytes_for() == coder.max_file_bytes
    assert coder.encode(planes_of([j]), 100, progressive=True) == ([data], [0])


@pytest.mark.parametrize("ncomp", [1, 3])
def test_synthetic_planes_cut_every_15_blocks(ncomp):
    j = synthetic_planes(ncomp)
    want = host_writer(j, 90, progressive=True)
    files, status = coder_for(j, 1).encode(planes_of([j]), 90, progressive=True)
    assert status == [0] and files[0] == want
    Image.open(io.BytesIO(files[0])).load()


def test_batch_of_different_images_and_alternating_flags():
    """Six images per call, three calls on one stage with other flags each, 0 among them: every call leaves the streams clean."""
    w, h, q = 320, 200, 85
    coder = None
    for call, flags in enumerate((2, 0, 1)):
        imgs = [photo(w, h, 100 * call + k, noise=10 + 20 * k) for k in range(6)]
        js = [twin(im, q, "4:2:0") for im in imgs]
        coder = coder or coder_for(js[0], 6)
        files, status = coder.encode(planes_of(js), q, **kw(flags))
        assert status == [0] * 6
        assert files == [save(im, q, "4:2:0", **(FLAGS[flags] if flags else {"optimize": False})) for im in imgs]
        if flags == 0:
            assert files == coder.encode(planes_of(js), q)[0]


@pytest.mark.parametrize("flags", [1, 2])
def test_dropped_images_leave_the_others_alone(flags):
    w, h, q = 96, 64, 90
    imgs = [photo(w, h, k) for k in range(4)]
    datas = [save(im, q, "4:4:4", **FLAGS[flags]) for im in imgs]
    js = [twin(im, q, "4:4:4") for im in imgs]
    good = js[2]["coef"][1]
    js[2]["coef"][1] = good.copy()
    # 11 magnitude bits where the range is checked: as it stands in the sequential scan, after the first AC scan's shift by one
    js[2]["coef"][1].reshape(-1)[64 * 7 + 9] = -1500 if flags == 1 else -3000
    coder = coder_for(js[0], 4)
    files, status = coder.encode(planes_of(js), q, **kw(flags))
    assert status == [0, 0, M.ENC_BAD_COEFFICIENT, 0]
    assert files == [datas[0], datas[1], None, datas[3]]
    js[2]["coef"][1] = good
    longest = max(len(d) for d in datas)                                         # file_pitch one byte short for the longest file
    files, status = coder.encode(planes_of(js), q, file_pitch=max(longest - 1, 1024), **kw(flags))
    for d, f, s in zip(datas, files, status):
        assert (f, s) == ((None, M.ENC_FILE_OVERFLOW) if len(d) == longest else (d, 0))
    assert coder.encode(planes_of(js), q, **kw(flags)) == (datas, [0] * 4)       # the stage is clean afterwards
    small = coder_for(js[0], 4, scan_capacity=4096)
    files, status = small.encode(planes_of(js), q, **kw(flags))
    for d, f, s in zip(datas, files, status):
        assert s in (0, M.ENC_SCAN_OVERFLOW) and (f == d if s == 0 else f is None)
    assert small.encode(planes_of(js), q, **kw(flags)) == (files, status)


@pytest.mark.parametrize("pitch_of", [lambda longest: 1024, lambda longest: (longest // 2) & ~15, lambda longest: (longest - 16) & ~15])
def test_files_that_do_not_fit_never_write_behind_their_slot(pitch_of):
    rng = np.random.default_rng(5)
    w, h, q = 200, 152, 100
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if k % 2 else photo(w, h, k) for k in range(6)]
    datas = [save(im, q, "4:2:0", progressive=True) for im in imgs]
    js = [twin(im, q, "4:2:0") for im in imgs]
    longest = max(len(d) for d in datas)
    pitch = pitch_of(longest)
    coder = coder_for(js[0], 6)
    guard = 1 << 20
    buf = torch.full((6 * pitch + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    files, lengths, status = coder.encode_device(planes_of(js), q, file_pitch=pitch, files=buf[:6 * pitch].view(6, pitch), progressive=True)
    torch.cuda.synchronize()
    assert bool((buf[6 * pitch:] == 0xA5).all()), "a byte landed behind the last slot"
    lengths, status, host = lengths.cpu().numpy(), status.cpu().numpy(), files.cpu().numpy()
    for i, d in enumerate(datas):
        if len(d) <= pitch:
            assert status[i] == 0 and host[i, :lengths[i]].tobytes() == d, i
        else:
            assert status[i] == M.ENC_FILE_OVERFLOW and lengths[i] == 0, i


def _frames(w, h, n):
    stride = O.stride_for_width(w)
    frames = np.zeros((n, h, stride), np.uint8)
    for k in range(n):
        rgb = photo(w, h, 50 + k, noise=5 + 25 * k)
        px = frames[k, :, :4 * w].reshape(h, w, 4)
        px[..., 0], px[..., 1], px[..., 2], px[..., 3] = rgb[..., 2], rgb[..., 1], rgb[..., 0], 255
    return frames, stride


def test_forward_stage_plus_device_coder_equals_host_writer():
    hs, vs = [2, 1, 1], [2, 1, 1]
    w, h, n, q = 801, 451, 5, 90
    frames, stride = _frames(w, h, n)
    stage = M.JpegForwardStage(w, h, hs, vs, n)
    qt = torch.from_numpy(np.stack([M.quant_tables_for_quality(q)] * n).view(np.int16)).cuda()
    coef = stage.write_frames(Bitmap.from_numpy(frames, w, h, stride, "cuda:0"), qt)
    coder = M.JpegEntropyStage(w, h, hs, vs, stage.blocks_w, stage.blocks_h, n)
    host_planes = [c.cpu().numpy() for c in coef]
    for opt in (False, True):
        files, status = coder.encode(coef, q, progressive=True, optimize_coding=opt)
        assert status == [0] * n
        assert files == M.write_jpeg_batch(host_planes, w, h, hs, vs, q, progressive=True, optimize_coding=opt)


def test_encoder_mirror_uses_the_device_coder_for_progressive():
    w, h, n = 200, 120, 3
    stride = O.stride_for_width(w)
    frames = np.random.default_rng(4).integers(0, 256, (n, h, stride), dtype=np.uint8)
    enc = M.MozjpegEncoder.create_classic(quality=88, progressive=True)
    on_device = enc.write_frames(Bitmap.from_numpy(frames.copy(), w, h, stride, "cuda:0"))
    on_host = enc.write_frames(Bitmap.from_numpy(frames.copy(), w, h, stride, "cuda:0"), device_entropy=False)
    assert on_device == on_host and all(b"\xff\xc2" in f[:400] and f[-2:] == b"\xff\xd9" for f in on_device)


@pytest.mark.parametrize("extra,pillow", [({"progressive": True}, {"progressive": True}),
                                          ({"optimize_huffman_coding": True}, {"optimize": True}),
                                          ({"progressive": True, "optimize_huffman_coding": True}, {"progressive": True, "optimize": True})])
def test_shim_codes_the_options_on_the_device_when_switched_on(extra, pillow):
    from imageflow_amd.abi import Context
    from tests import util as U
    from tests.test_gpu_abi_shim import _run, pack_raw_bgra
    w, h = 203, 131
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) * 3 % 256], -1).astype(np.int32)
    rgb = np.clip(rgb + rng.integers(-30, 30, rgb.shape), 0, 255).astype(np.uint8)
    bgra = np.zeros((h, U.stride_for(w)), np.uint8)
    bgra[:, :4 * w] = np.concatenate([rgb[:, :, ::-1], np.full((h, w, 1), 255, np.uint8)], -1).reshape(h, 4 * w)
    job = {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": {"libjpeg_turbo": dict(quality=88, **extra)}}}]}}
    want = save(rgb, 88, "4:2:0", **pillow)
    for on, counted in ((True, 1), (False, 0)):                    # a fresh context without the switch still counts 0
        with Context() as c:
            if on:
                assert c.set_device_jpeg_options(True)
            c.add_input_buffer(0, pack_raw_bgra(bgra, w, h, alpha_meaningful=False))
            c.add_output_buffer(1)
            _run(c, "v1/execute", job)
            assert bytes(c.get_output_buffer(1)) == want
            assert c.L.ifhip_shim_device_coded_files(c.p) == counted
