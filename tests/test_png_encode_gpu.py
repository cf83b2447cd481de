"""GPU suite: the device PNG encoder (csrc/png_encode.hip) against the format's statement in tests/png_encode_ref.py, byte for byte,
on every case of tests/png_encode_cases.py; slots are left clean; what the encoder cannot take is refused before any launch."""
import numpy as np
import pytest
import torch

import png_encode_cases
import png_encode_ref as ref

pytestmark = pytest.mark.gpu

CASES = png_encode_cases.cases()


@pytest.fixture(scope="module")
def ctx():
    from co_fusion_amd import api
    c = api.Context(64, 48, 50.0, 50.0, 32.0, 24.0, max_models=1, max_surfels=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference():
    return {name: ref.encode(img, ch, R, flags) for name, img, ch, R, flags in CASES}


def _file(st, bands):
    """the host writer's part in Python: the bands in order, the Adler-32 combined over the band table"""
    adler = 1
    for _, a, n in bands:
        adler = ref.adler32_combine(adler, a, n)
    return ref.assemble(st.width, st.height, st.channels, [b for b, _, _ in bands], adler)


def _encode(ctx, img, R, flags, slots=2, slot=0, times=1, offset=0):
    from co_fusion_amd import api
    h, w = img.shape[:2]
    enc = api.PngEncoder(ctx, w, h, slots=slots, rows_per_band=R)
    try:
        flat = torch.zeros(img.size + offset + 3, dtype=torch.uint8, device=ctx.device)
        flat[offset:offset + img.size] = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).to(ctx.device)
        dev = flat[offset:offset + img.size].view(*img.shape)
        out = []
        for _ in range(times):
            enc.submit(slot, dev, flags)
            out.append(_file(*enc.acquire(slot)))
        return out
    finally:
        enc.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_stream_equals_the_reference(ctx, reference, case):
    name, img, ch, R, flags = case
    want, trace = reference[name]
    got, = _encode(ctx, img, R, flags)
    assert len(got) == len(want), (name, len(got), len(want), [b["kind"] for b in trace["bands"]])
    assert got == want, (name, "first difference at byte", next(i for i in range(len(want)) if got[i] != want[i]),
                         "bands", [(b["kind"], b["bytes"]) for b in trace["bands"]][:8])


def test_source_at_any_byte_alignment(ctx, reference):
    """the rows are loaded as aligned words: an image that starts 1, 2 or 3 bytes into a word encodes the same"""
    name, img, ch, R, flags = next(c for c in CASES if c[0] == "label_blobs_67x12")
    for offset in (1, 2, 3):
        got, = _encode(ctx, img, R, flags, offset=offset)
        assert got == reference[name][0], offset


def test_slots_are_left_clean(ctx, reference):
    """a big image, then a small one, twice through one slot and through another slot of a larger encoder"""
    from co_fusion_amd import api
    by = {c[0]: c for c in CASES}
    enc = api.PngEncoder(ctx, 67, 16, slots=3, rows_per_band=5)
    try:
        def run(slot, name, R=5):
            _, img, ch, _, flags = by[name]
            dev = torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)
            enc.submit(slot, dev, flags)
            torch.cuda.synchronize()
            want = ref.encode(img, ch, R, flags)[0]
            return _file(*enc.acquire(slot)) == want
        assert run(0, "noise_rgba_65x9")
        assert run(0, "label_blobs_67x12") and run(0, "label_blobs_67x12")
        assert run(2, "label_blobs_67x12")
        assert run(0, "grey_1x1") and run(2, "zero_rgba_64x16") and run(0, "noise_rgba_65x9")
        # two submits in a row to one slot, no acquire in between: the second image is what the slot holds
        a = torch.from_numpy(by["noise_rgba_65x9"][1]).to(ctx.device)
        b = torch.from_numpy(by["label_blobs_67x12"][1]).to(ctx.device)
        enc.submit(1, a, 0)
        enc.submit(1, b, ref.CF_PNG_LABELS)
        assert _file(*enc.acquire(1)) == ref.encode(by["label_blobs_67x12"][1], 1, 5, ref.CF_PNG_LABELS)[0]
    finally:
        enc.close()


def test_timing_counts_images(ctx):
    from co_fusion_amd import api
    enc = api.PngEncoder(ctx, 64, 16, slots=2, rows_per_band=8)
    try:
        enc.timing(True)
        dev = torch.zeros((16, 64, 4), dtype=torch.uint8, device=ctx.device)
        for s in (0, 1, 0):
            enc.submit(s, dev)
        ms, n = enc.timing(False)
        assert n == 3 and ms > 0
        assert enc.timing(False) == (0.0, 0)
    finally:
        enc.close()


def test_refusals_launch_nothing(ctx):
    from co_fusion_amd import api
    lib = ctx.lib
    for args in ((1280, 2, 2, 13), (64, 16, 2, 0), (64, 16, 1, 8), (64, 16, 17, 8), (0, 16, 2, 8), (16383, 1, 2, 2)):
        with pytest.raises(api.CofusionError, match="error -1"):   # CF_EINVAL
            api.PngEncoder(ctx, args[0], args[1], slots=args[2], rows_per_band=args[3])
    enc = api.PngEncoder(ctx, 32, 8, slots=2, rows_per_band=4)
    try:
        ok = torch.zeros((8, 32), dtype=torch.uint8, device=ctx.device)
        enc.submit(0, ok)
        first = _file(*enc.acquire(0))
        for shape, flags in (((9, 32), 0), ((8, 33), 0), ((8, 32, 3), 0), ((8, 32, 4), ref.CF_PNG_LABELS), ((8, 32), 2)):
            with pytest.raises(api.CofusionError, match="error -1"):
                enc.submit(0, torch.full(shape, 9, dtype=torch.uint8, device=ctx.device), flags)
        with pytest.raises(api.CofusionError, match="error -1"):
            enc.submit(2, ok)
        with pytest.raises(api.CofusionError, match="error -1"):
            enc.submit_ptr(0, 0, 32, 8, 1)
        with pytest.raises(api.CofusionError, match="error -4"):   # CF_ESTATE: nothing was submitted to slot 1
            enc.acquire(1)
        torch.cuda.synchronize()
        assert _file(*enc.acquire(0)) == first   # the slot still holds the accepted image: a refused submit touched nothing
        assert lib.cf_png_encoder_submit(None, 0, None, 1, 1, 1, 0) == -1
    finally:
        enc.close()
