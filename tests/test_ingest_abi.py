"""CPU: the frame-ingest library (libclipfsar_ingest.so, include/clipfsar_ingest.h) validates arguments and descriptor tables without a GPU;
FrameIngest, StreamPool.push_u8 and WindowStream.push_u8 reject misuse before any device work.  Its exports, kernels and place in the build
are checked with every library's in tests/test_build_recipe.py."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import pytest

from _abi import check_abi_at_load, check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_ingest.h")


@pytest.fixture(scope="module")
def ilib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import ingest_hip
    return ingest_hip.lib()


def test_header_exported_exactly_and_arity_matches(ilib):
    check_exports(lib_row("ingest"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import ingest_hip as ih
    text = open(HEADER).read()
    assert int(re.search(r"#define CFSI_MAX_GROUPS (\d+)", text).group(1)) == ih.MAX_GROUPS
    assert int(re.search(r"#define CFSI_SRC_ALIGN (\d+)", text).group(1)) == ih.SRC_ALIGN == 16
    assert int(re.search(r"#define CFSI_TABLE_COLS (\d+)", text).group(1)) == ih.TABLE_COLS == 9
    cols = ("SRC_OFF16", "N", "OUT_OFF", "H", "W", "SCALE_H", "SCALE_W", "Y0", "X0")
    for i, col in enumerate(cols):                # the binding's column order is the header's
        assert int(re.search(r"#define CFSI_%s (\d+)" % col, text).group(1)) == getattr(ih, col) == i


def test_abi_version_is_checked_at_load(ilib, monkeypatch):
    check_abi_at_load(lib_row("ingest"), monkeypatch)


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        src_off16 n out_off H    W   sh   sw  y0  x0
GOOD = [[0,        2, 0,     10,  16, 40,  48, 4,  8],        # 2 * 10 * 16 * 3 = 960 bytes at 0
        [60,       1, 2,     2,   2,  40,  48, 4,  8],        # 12 bytes at 960
        [64,       3, 3,     7,   5,  40,  48, 4,  8]]        # 315 bytes at 1024 .. 1339; N = 6, crop 32
BYTES = 1339


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_argument_validation_without_gpu(ilib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good = ilib.cfsi_last_error, _tbl(GOOD)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ms = ctypes.cast(f3, ctypes.c_void_p)
    tf = ilib.cfsi_transform_frames

    # transform_frames(src, src_bytes, out, table_host, table_dev, S, N, crop, mean3, std3, stream)
    def call(table=good, S=3, N=6, crop=32, nbytes=BYTES, src=p, out=p, tdev=p, mean=ms, std=ms):
        return tf(src, nbytes, out, table, tdev, S, N, crop, mean, std, None)

    for kw in ({"src": None}, {"out": None}, {"table": None}, {"tdev": None}, {"mean": None}, {"std": None}):
        assert call(**kw) != 0 and b"null" in err(), kw
    for kw in ({"N": 0}, {"crop": 0}, {"nbytes": 0}, {"N": -3}):
        assert call(**kw) != 0 and b"bad shape" in err(), kw
    zero = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    assert call(std=ctypes.cast(zero, ctypes.c_void_p)) != 0 and b"std of 0" in err()
    for S in (0, -1, 1 << 17):
        assert call(S=S) != 0 and b"rows" in err(), S
    assert call(table=_edit(1, 1, 0)) != 0 and b"at least 1" in err()                            # a row with n = 0
    assert call(table=_edit(1, 1, -2)) != 0 and b"at least 1" in err()
    for col in (3, 4):                                                                           # H = 1, W = 1
        assert call(table=_edit(0, col, 1)) != 0 and b"at least 2" in err(), col
    for col in (5, 6):                                                                           # scale below crop
        assert call(table=_edit(2, col, 31)) != 0 and b"below crop" in err(), col
    assert call(crop=41) != 0 and b"below crop" in err()
    for col, v in ((7, -1), (8, -1), (7, 9), (8, 17)):                                           # 9 + 32 > 40, 17 + 32 > 48
        assert call(table=_edit(0, col, v)) != 0 and b"crop window" in err() and b"outside" in err(), (col, v)
    for row, v in ((1, 1), (2, 4), (0, 1)):                                                      # a prefix offset that is not the running sum
        assert call(table=_edit(row, 2, v)) != 0 and b"prefix sum" in err(), (row, v)
    assert call(N=7) != 0 and b"not to N" in err()
    assert call(S=2) != 0 and b"not to N" in err()
    assert call(nbytes=BYTES - 1) != 0 and b"beyond src_bytes" in err()                          # the last group ends one byte late
    assert call(table=_edit(0, 0, 24)) != 0 and b"beyond src_bytes" in err()                     # 384 + 960 > 1339
    assert call(table=_edit(0, 1, 3)) != 0                                                       # (n = 3 also breaks the prefix sums)
    assert call(table=_edit(1, 0, -1)) != 0 and b"negative source offset" in err()
    assert call(table=_tbl([[0, 1, 0, 40000, 40000, 40, 48, 4, 8]]), S=1, N=1, nbytes=1 << 40) != 0 and b"32-bit" in err()
    assert call(table=_tbl([[0, 1, 0, 4, 4, 1 << 20, 1 << 20, 0, 0]]), S=1, N=1, crop=1 << 15, nbytes=48) != 0 and b"too large" in err()


def test_python_wrappers_reject_cpu_tensors_and_bad_tables(ilib):
    import torch
    from clip_fsar_amd import ingest_hip as ih
    from clip_fsar_amd import pool_hip as ph
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ph.Table(host, host, 3)               # a device copy that is no device tensor
    src, out = torch.zeros(BYTES, dtype=torch.uint8), torch.zeros(6, 3, 32, 32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ih.transform_frames(src, out, table, 32, (0.5,) * 3, (0.5,) * 3)
    with pytest.raises(RuntimeError, match="shape"):
        ih.transform_frames(src, out, table, 28, (0.5,) * 3, (0.5,) * 3)
    with pytest.raises(RuntimeError, match="Table"):
        ih.transform_frames(src, out, ph.Table(host[:, :8], host, 3), 32, (0.5,) * 3, (0.5,) * 3)
    up = ih.table_uploader("cpu", 4)
    assert up.cols == ih.TABLE_COLS and ph.TableUploader("cpu", 4).cols == ph.TABLE_COLS == 8       # the pool's uploader is what it was
    with pytest.raises(RuntimeError, match="1 .. 4 rows of 9"):
        up.upload([[0] * 8])


# ------------------------------------------------------------------ FrameIngest and the push_u8 entry points: misuse, before any device work
MEAN, STD = (0.4, 0.5, 0.6), (0.2, 0.3, 0.4)


def test_frame_ingest_rejects_misuse_before_any_launch():
    import torch
    from clip_fsar_amd.ingest import FrameIngest
    for kw in ({"test_scale": 200}, {"test_scale": [256, 100]}, {"crop": 0}, {"crop": 2.5}, {"depth": 0}, {"std": (1.0, 0.0, 1.0)},
               {"mean": (1.0, 2.0)}, {"test_scale": "big"}):
        with pytest.raises(ValueError):
            FrameIngest(**dict({"device": "cpu", "test_scale": 256, "crop": 224, "mean": MEAN, "std": STD}, **kw))
    fi = FrameIngest("cpu", 256, 224, MEAN, STD)
    ok = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for bad in ([], (), None, ok):
        with pytest.raises(ValueError, match="non-empty list"):
            fi.transform(bad)
    with pytest.raises(TypeError, match="not a tensor"):
        fi.transform([ok, "clip"])
    with pytest.raises(TypeError, match="uint8"):
        fi.transform([ok, torch.zeros(2, 8, 8, 3)])                           # CPU fp32 frames
    with pytest.raises(TypeError, match="uint8"):
        fi.transform([torch.zeros(2, 8, 8, 3, dtype=torch.int8)])
    for shape in ((8, 8, 3), (1, 2, 8, 8, 3), (2, 3, 8, 8), (2, 8, 8, 4)):     # wrong rank, last dim not 3
        with pytest.raises(ValueError, match=r"\[n, H, W, 3\]"):
            fi.transform([torch.zeros(*shape, dtype=torch.uint8)])
    for shape in ((0, 8, 8, 3), (2, 1, 8, 3), (2, 8, 1, 3)):
        with pytest.raises(ValueError, match="H, W >= 2"):
            fi.transform([ok, torch.zeros(*shape, dtype=torch.uint8)])
    assert fi.check([ok, torch.zeros(1, 5, 9, 3, dtype=torch.uint8)]) == [(2, 8, 8), (1, 5, 9)]
    with pytest.raises(RuntimeError, match="no CPU path"):                    # a well-formed call on an ingest without a device
        fi.transform([ok])
    assert fi._copy_stream is None and all(s.dev is None for s in fi._slots)  # nothing was staged by any of the above


def test_from_cfg_reads_the_data_section():
    from clip_fsar_amd.ingest import FrameIngest
    cfg = NS(DATA=NS(TEST_SCALE=[72, 96], TEST_CROP_SIZE=64, MEAN=list(MEAN), STD=list(STD), NUM_INPUT_FRAMES=8))
    fi = FrameIngest.from_cfg(cfg, "cpu")
    assert (fi.scale_hw, fi.crop, fi.mean, fi.std, fi.depth) == ((72, 96), 64, MEAN, STD, 2)
    assert FrameIngest.from_cfg(NS(DATA=NS(TEST_SCALE=256, TEST_CROP_SIZE=224, MEAN=MEAN, STD=STD)), "cpu").scale_hw == (256, 256)
    with pytest.raises(ValueError, match=r"DATA\.TEST_SCALE, DATA\.TEST_CROP_SIZE"):
        FrameIngest.from_cfg(NS(DATA=NS(NUM_INPUT_FRAMES=8, MEAN=MEAN, STD=STD)), "cpu")


def _stub_head(T=4, **train):                     # tests/test_pool_abi.py's stub: its DATA section has no TEST_SCALE
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def test_push_u8_errors_on_a_stub_head():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.ingest import FrameIngest
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    gal = SupportGallery(_stub_head(), "cpu")
    lazy = StreamPool(gal, max_streams=3)         # no DATA.TEST_SCALE: the pool is built all the same
    assert lazy._ingest is None
    with pytest.raises(TypeError, match="FrameIngest"):
        StreamPool(gal, ingest="ingest")
    with pytest.raises(TypeError, match="FrameIngest"):
        WindowStream(gal, ingest=3)
    u8 = torch.zeros(2, 6, 10, 3, dtype=torch.uint8)
    a = lazy.open()
    with pytest.raises(RuntimeError, match="no classes registered"):
        lazy.push_u8({a: u8})
    gal._ids.append(0)                            # a registered class: the pushes get as far as their own checks
    with pytest.raises(ValueError, match=r"lacks DATA\.TEST_SCALE"):
        lazy.push_u8({a: u8})                     # only now is the config asked for the transform
    fi = FrameIngest("cpu", 8, 4, MEAN, STD)
    p = StreamPool(gal, max_streams=3, ingest=fi)
    assert p.ingest is fi
    a, b, c = p.open(), p.open(), p.open()
    p.close(b)
    before = [p.stats(h) for h in (a, c)] + [p.stats()]
    with pytest.raises(ValueError, match="not open"):
        p.push_u8({a: u8, b: u8})                 # a closed handle
    with pytest.raises(ValueError, match="not open"):
        p.push_u8_packed([u8, u8], [a, 17])
    with pytest.raises(ValueError, match="appears twice"):
        p.push_u8_packed([u8, u8], [a, a])
    with pytest.raises(ValueError, match="2 clips for 1 sessions"):
        p.push_u8_packed([u8, u8], [a])
    with pytest.raises(TypeError, match="uint8"):
        p.push_u8({a: u8, c: u8.float()})         # CPU fp32 frames
    with pytest.raises(TypeError, match="uint8"):
        p.push_u8_packed([u8.to(torch.int16)], [a])
    with pytest.raises(ValueError, match=r"\[n, H, W, 3\]"):
        p.push_u8({a: u8[0]})
    with pytest.raises(ValueError, match="H, W >= 2"):
        p.push_u8({a: u8[:0]})                    # no frames
    for bad in ({}, [u8], None):
        with pytest.raises(ValueError, match="non-empty dict"):
            p.push_u8(bad)
    with pytest.raises(ValueError, match="non-empty list"):
        p.push_u8_packed([], [])
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.push_u8({a: u8})                        # well-formed, but this pool has no device
    assert [p.stats(h) for h in (a, c)] + [p.stats()] == before and fi._copy_stream is None
    # WindowStream.push_u8: [B, n, H, W, 3]
    ws = WindowStream(gal, n_streams=2, ingest=fi)
    for bad in (u8, torch.zeros(3, 2, 6, 10, 3, dtype=torch.uint8), torch.zeros(2, 0, 6, 10, 3, dtype=torch.uint8), None):
        with pytest.raises(ValueError, match=r"\[B, n, H, W, 3\] with B = 2"):
            ws.push_u8(bad)
    with pytest.raises(TypeError, match="uint8"):
        ws.push_u8(torch.zeros(2, 2, 6, 10, 3))
    with pytest.raises(ValueError, match=r"\[n, H, W, 3\]"):
        ws.push_u8(torch.zeros(2, 2, 6, 10, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ws.push_u8(torch.zeros(2, 2, 6, 10, 3, dtype=torch.uint8))
    assert ws.stats == {"frames": 0, "tower_frames": 0, "windows": 0}
    with pytest.raises(ValueError, match=r"lacks DATA\.TEST_SCALE"):
        WindowStream(gal, n_streams=2).push_u8(torch.zeros(2, 2, 6, 10, 3, dtype=torch.uint8))


def test_an_ingest_that_does_not_fit_the_tower_is_rejected_before_the_clips_are_looked_at():
    """another device: at construction; a crop other than the tower's input resolution: by push_u8, before the upload"""
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.ingest import FrameIngest
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    head = _stub_head()
    head._get_engine(None).arch["res"] = 8        # a tower of 8 x 8 frames
    gal = SupportGallery(head, "cpu")
    gal._ids.append(0)
    for cls in (StreamPool, WindowStream):
        with pytest.raises(ValueError, match="the ingest lives on cuda:0, the gallery on cpu"):
            cls(gal, ingest=FrameIngest("cuda:0", 8, 8, MEAN, STD))
    fi = FrameIngest("cpu", 8, 4, MEAN, STD)
    fi.serves("cpu", 4)
    fi.serves(torch.device("cpu"))
    p = StreamPool(gal, max_streams=2, ingest=fi)
    a = p.open()
    with pytest.raises(ValueError, match="crops to 4 x 4, the tower takes 8 x 8"):
        p.push_u8({a: "not even a clip"})
    with pytest.raises(ValueError, match="crops to 4 x 4, the tower takes 8 x 8"):
        WindowStream(gal, n_streams=1, ingest=fi).push_u8(None)
    assert p.stats(a)["frames"] == 0 and fi._copy_stream is None
    fits = StreamPool(gal, max_streams=2, ingest=FrameIngest("cpu", 8, 8, MEAN, STD))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fits.push_u8({fits.open(): torch.zeros(2, 6, 10, 3, dtype=torch.uint8)})
