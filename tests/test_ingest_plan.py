"""CPU: plan_ingest, the host plan of a FrameIngest.transform call, with no kernel involved.  The golden cases of the frame transform that
share a crop size are packed as the groups of one plan; the test then does what the kernel does with a table row -- slice the staging
bytes by the row's offset and n * H * W * 3, transform them with the row's geometry (through the CPU oracle) -- and compares with the
golden from the reference at the oracle's own bound.  Random shape lists: aligned offsets, non-overlapping groups, exact totals."""
import collections
import random

import pytest
import torch

import clip_fsar_amd.synth as synth
import clipfsar_oracle as orc
from clip_fsar_amd import ingest_hip as ih
from clip_fsar_amd.ingest import ALIGN, plan_ingest, scale_hw
from clip_fsar_amd.preprocess import crop_window
from test_preprocess_n2 import _cases

CPU_BOUND = 1e-6          # tests/test_preprocess_n2.py::test_oracle_preprocess_matches_reference


def _staged(plan, clips, fill=0xAB):
    """the staging buffer of a plan: every clip's bytes at its offset, the padding between them filled with a value no result may show"""
    buf = torch.full((plan.total_bytes,), fill, dtype=torch.uint8)
    for off, c in zip(plan.offsets, clips):
        buf[off:off + c.numel()] = c.reshape(-1)
    return buf


def _interpret(plan, buf):
    """what the kernel computes from the table and the staging bytes, through the oracle: [N, 3, crop, crop]"""
    out = torch.full((plan.n_frames, 3, plan.crop, plan.crop), float("nan"))
    for row in plan.rows:
        n, H, W = row[ih.N], row[ih.H], row[ih.W]
        first = row[ih.SRC_OFF16] * ih.SRC_ALIGN
        frames = buf[first:first + n * H * W * 3].view(n, H, W, 3)
        out[row[ih.OUT_OFF]:row[ih.OUT_OFF] + n] = orc.preprocess_frames(frames, [row[ih.SCALE_H], row[ih.SCALE_W]], plan.crop, row[ih.Y0],
                                                                         row[ih.X0], synth.CLIP_MEAN, synth.CLIP_STD)
    return out


def test_plan_of_the_golden_cases_against_the_reference():
    by_crop = collections.defaultdict(list)
    for name, c, vid, scale, ref in _cases():
        by_crop[(c["crop"], tuple(scale), c["nsc"])].append((name, c, vid, ref))
    assert max(len(v) for v in by_crop.values()) >= 2               # at least one plan with several groups of different geometry
    for (crop, scale, nsc), group in by_crop.items():
        clips = [vid for _, _, vid, _ in group]
        test_scale = scale[0] if scale[0] == scale[1] else list(scale)
        plan = plan_ingest([c.shape[:3] for c in clips], test_scale, crop, nsc, [c["idx"] for _, c, _, _ in group])
        assert plan.n_frames == sum(c.shape[0] for c in clips) and plan.crop == crop and plan.scale_hw == scale
        got = _interpret(plan, _staged(plan, clips))
        want = torch.cat([ref for _, _, _, ref in group])
        assert got.shape == want.shape and not torch.isnan(got).any()
        err = float((got - want).abs().max())
        print("plan of %s: |interpreted rows - reference golden| = %.2e" % ([n for n, _, _, _ in group], err))
        assert err < CPU_BOUND, ([n for n, _, _, _ in group], err)
        # the groups in the other order, and with a coarser alignment: other offsets, the same frames
        rev = plan_ingest([c.shape[:3] for c in clips[::-1]], test_scale, crop, nsc, [c["idx"] for _, c, _, _ in group][::-1], align=4096)
        got = _interpret(rev, _staged(rev, clips[::-1]))
        want = torch.cat([ref for _, _, _, ref in group[::-1]])
        assert float((got - want).abs().max()) < CPU_BOUND


def test_scale_rule_and_crop_window_columns():
    assert scale_hw(256) == (256, 256) and scale_hw([72, 96]) == (72, 96) and scale_hw((96, 72)) == (96, 72)
    for bad in (256.0, [72], [72, 96, 3], "256", None, True, [72.0, 96]):
        with pytest.raises(ValueError, match="TEST_SCALE"):
            scale_hw(bad)
    plan = plan_ingest([(3, 240, 320), (1, 97, 131)], 256, 224)
    for row in plan.rows:
        assert row[ih.SCALE_H:ih.X0 + 1] == [256, 256, 16, 16]
    plan = plan_ingest([(3, 240, 320), (1, 97, 131)], [72, 96], 64, 3, [0, 2])
    assert [r[ih.Y0:ih.X0 + 1] for r in plan.rows] == [list(crop_window((72, 96), 64, 3, 0)), list(crop_window((72, 96), 64, 3, 2))]
    assert [r[ih.Y0:ih.X0 + 1] for r in plan.rows] == [[4, 0], [4, 32]]
    for kw in ({"test_scale": 200}, {"test_scale": [256, 128]}, {"crop": 0}, {"align": 8}, {"align": 24}, {"shapes": []},
               {"shapes": [(0, 8, 8)]}, {"shapes": [(1, 1, 8)]}, {"shapes": [(1, 8, 1)]}, {"idx": [1]}):
        with pytest.raises(ValueError):
            plan_ingest(**dict({"shapes": [(1, 8, 8), (2, 9, 9)], "test_scale": 256, "crop": 224}, **kw))


@pytest.mark.parametrize("seed", range(6))
def test_random_shape_lists(seed):
    rng = random.Random(seed)
    align = rng.choice((16, 64, ALIGN, 4096))
    shapes = [(rng.randint(1, 17), rng.randint(2, 400), rng.randint(2, 700)) for _ in range(rng.randint(1, 40))]
    plan = plan_ingest(shapes, 256, 224, align=align)
    assert ALIGN % ih.SRC_ALIGN == 0 and len(plan.rows) == len(plan.offsets) == len(shapes)
    end, frames = 0, 0
    for (n, H, W), row, off in zip(shapes, plan.rows, plan.offsets):
        assert off % align == 0 and off % ih.SRC_ALIGN == 0 and row[ih.SRC_OFF16] * ih.SRC_ALIGN == off
        assert end <= off < end + align                             # behind the group before, no further than the alignment asks
        assert row[ih.N:ih.W + 1] == [n, frames, H, W]
        end, frames = off + n * H * W * 3, frames + n
    assert plan.total_bytes == end and plan.n_frames == frames      # exact: no padding behind the last group
    assert all(len(r) == ih.TABLE_COLS and all(isinstance(v, int) and 0 <= v < 2 ** 31 for v in r) for r in plan.rows)
