"""Property tests for the pure-NumPy image codecs (hypothesis): random
sizes / qualities / content / filter choices, cross-validated against
PIL (libjpeg + its PNG encoder) as the independent oracle."""
import io

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

PIL = pytest.importorskip("PIL.Image")

from raft_amd.data.jpeg import decode_jpeg, encode_jpeg


@settings(max_examples=12, deadline=None)
@given(h=st.integers(8, 70), w=st.integers(8, 70),
       q=st.integers(40, 98), sub=st.sampled_from([0, 1, 2]),
       seed=st.integers(0, 2**31))
def test_encode_is_standard_and_self_consistent(h, w, q, sub, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    enc = encode_jpeg(img, quality=q, subsampling=sub)
    mine = decode_jpeg(enc)
    assert mine.shape == img.shape
    # PIL decodes my bitstream to (essentially) the same pixels
    pil = np.asarray(PIL.open(io.BytesIO(enc)).convert("RGB"))[:, :, ::-1]
    d = np.abs(mine.astype(int) - pil.astype(int))
    assert d.mean() < (1.5 if sub == 0 else 4.0), (sub, d.mean())


@settings(max_examples=10, deadline=None)
@given(h=st.integers(9, 60), w=st.integers(9, 60),
       sub=st.sampled_from([0, 1, 2]), q=st.integers(55, 95),
       prog=st.booleans(), seed=st.integers(0, 2**31))
def test_decode_arbitrary_pil_streams(h, w, sub, q, prog, seed):
    rng = np.random.default_rng(seed)
    # smooth + structured content (pure noise is a worst case for chroma
    # subsampling in ANY decoder; covered at 4:4:4 by the test above)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 90 * np.sin(yy / 5), 128 + 90 * np.cos(xx / 7),
                    128 + 50 * np.sin((xx + yy) / 6)], axis=2)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    PIL.fromarray(img).save(buf, "JPEG", quality=q, subsampling=sub,
                            progressive=prog)
    mine = decode_jpeg(buf.getvalue())
    pil = np.asarray(PIL.open(io.BytesIO(buf.getvalue())).convert("RGB")) \
        [:, :, ::-1]
    d = np.abs(mine.astype(int) - pil.astype(int))
    assert d.mean() < (1.2 if sub == 0 else 4.0), (sub, d.mean())


@settings(max_examples=12, deadline=None)
@given(h=st.integers(4, 80), w=st.integers(4, 80),
       mode=st.sampled_from(["RGB", "L", "RGBA", "P"]),
       interlace=st.booleans(), seed=st.integers(0, 2**31))
def test_png_decoder_against_pil_streams(h, w, mode, interlace, seed):
    """The pure-NumPy PNG decoder vs PIL-written files: external encoders
    pick adaptive scanline filters (sub/up/avg/paeth), exercising every
    unfilter path; palette and alpha variants included."""
    from raft_amd.data.imageio import decode_png
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    im = PIL.fromarray(rgb).convert(mode)
    buf = io.BytesIO()
    im.save(buf, "PNG", interlace=interlace)
    mine = decode_png(buf.getvalue())           # HxWx3 BGR
    ref = np.asarray(im.convert("RGB"))[:, :, ::-1]
    assert mine.shape == ref.shape
    assert np.array_equal(mine, ref)


@settings(max_examples=8, deadline=None)
@given(h=st.integers(4, 60), w=st.integers(4, 60),
       interlace=st.booleans(), seed=st.integers(0, 2**31))
def test_png_16bit_high_byte(h, w, interlace, seed):
    """16-bit grayscale PNGs decode to the high byte of each sample —
    cv2.imdecode's default 8-bit conversion, which the reference's
    dataflow relied on."""
    from raft_amd.data.imageio import decode_png
    rng = np.random.default_rng(seed)
    a16 = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    buf = io.BytesIO()
    PIL.fromarray(a16.astype(np.int32), "I").convert("I;16") \
        .save(buf, "PNG", interlace=interlace)
    mine = decode_png(buf.getvalue())
    hi = (a16 >> 8).astype(np.uint8)
    assert mine.shape == (h, w, 3)
    assert np.array_equal(mine[:, :, 0], hi)
    assert np.array_equal(mine[:, :, 0], mine[:, :, 2])


def test_png_decoder_on_system_files():
    """Real-world PNGs written by external tools (sub-byte bit depths
    are the only rejected class — loudly)."""
    import glob as _glob
    import os
    from raft_amd.data.imageio import decode_png
    # copies of gitweb / desktop-icon PNGs, stored with the tests
    candidates = sorted(_glob.glob(os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "golden", "images",
        "*.png")))
    assert len(candidates) == 3, candidates
    checked = 0
    for path in candidates[:8]:
        data = open(path, "rb").read()
        try:
            mine = decode_png(data)
        except ValueError as e:
            assert "bit" in str(e), (path, e)   # sub-byte depths rejected
            continue
        ref = np.asarray(PIL.open(io.BytesIO(data)).convert("RGB")) \
            [:, :, ::-1]
        assert np.array_equal(mine, ref), path
        checked += 1
    assert checked >= 1, "no decodable system PNGs found"


def test_encode_png_bgra_and_bad_channels():
    """4-channel input drops alpha (layer contract is BGR); other channel
    counts error loudly instead of writing a corrupt stream."""
    from raft_amd.data.imageio import decode_png, encode_png
    rng = np.random.default_rng(7)
    bgra = rng.integers(0, 256, (9, 11, 4), dtype=np.uint8)
    out = decode_png(encode_png(bgra))
    assert np.array_equal(out, bgra[:, :, :3])
    with pytest.raises(ValueError, match="ch"):
        encode_png(rng.integers(0, 256, (4, 4, 2), dtype=np.uint8))
