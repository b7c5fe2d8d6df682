"""tests/upscale_ref.py checked on inputs whose answers can be worked out by hand: each of the three stages of the rule of
include/drt.h is reached and gives what the rule says, the first tap wins a tie in stage 2, a NaN distance never wins, an image of
misses reduces to plain bilinear interpolation, and the made-up inputs of the kernel tests hold every case they are meant to."""
import numpy as np
import pytest

from tests import upscale_ref as up

EXACT0 = dict(up.EXACT, demodulate=0)


def guides(H, W, hit=True, normal=(0, 0, 1), t=1.0, albedo=(0.5, 0.5, 0.5)):
    g = up.Guides(np.tile(np.float32(albedo), (H, W, 1)), np.tile(np.float32(normal), (H, W, 1)), np.full((H, W), t, np.float32),
                  np.zeros((H, W), np.int32))
    if not hit:
        g.normal[:], g.t[:], g.prim[:] = 0, up.FLT_MAX, -1
    return g


def ramp(H, W):
    c = np.ones((H, W, 4), np.float32)
    c[..., 0] = np.arange(W, dtype=np.float32)[None, :] / 4
    c[..., 1] = np.arange(H, dtype=np.float32)[:, None] / 8
    c[..., 2] = 0.25
    return c


def test_stage_1_on_one_surface_is_bilinear_and_exact():
    """Equal guides everywhere: e = 0, w = b, so 2 x 2 -> 4 x 4 gives the weights 1, 1/2 | 1/2 of the pixel-corner convention."""
    c = ramp(2, 2)
    out, stage = up.upscale(c, guides(2, 2), guides(4, 4), stages=True, **EXACT0)
    assert (stage == 1).all() and (out[..., 3] == 1).all()
    assert out[0, :, 0].tolist() == [0.0, 0.125, 0.25, 0.25]            # fx = 0, 0.5, 1, 1.5; the tap right of the last column is clamped
    assert out[:, 0, 1].tolist() == [0.0, 0.0625, 0.125, 0.125]
    assert (out.view(np.uint32) == up.bilinear(c, 4, 4).view(np.uint32)).all()


def test_an_image_of_misses_reduces_to_plain_bilinear():
    rng = np.random.default_rng(5)
    c = np.concatenate([rng.random((5, 7, 3), np.float32), np.ones((5, 7, 1), np.float32)], axis=-1)
    lo, hi = guides(5, 7, hit=False), guides(11, 16, hit=False)
    lo.albedo[:] = rng.random((5, 7, 3), np.float32)                     # a miss's sky albedo plays no part when demodulate == 0
    out, stage = up.upscale(c, lo, hi, stages=True, demodulate=0)
    assert (stage == 1).all()
    assert (out.view(np.uint32) == up.bilinear(c, 16, 11).view(np.uint32)).all()


def test_stage_1_weighs_a_tap_by_its_distance_and_drops_it_beyond_16():
    c = np.ones((1, 2, 4), np.float32)
    c[0, 0, :3], c[0, 1, :3] = 0, 1
    lo, hi = guides(1, 2), guides(1, 4)
    lo.t[0, 1] = 1.5                                                    # dz = 0.5 / 0.25 = 2, e = 4 against the output pixels (t = 1)
    out, stage = up.upscale(c, lo, hi, stages=True, **EXACT0)
    w = np.float32(0.5) * np.exp(np.float32(-4))
    assert (stage == 1).all() and out[0, 1, 0] == w / (np.float32(0.5) + w)
    lo.t[0, 1] = 2                                                      # dz = 4, e = 16: still accepted
    d = up.upscale(c, lo, hi, details=True, **EXACT0)
    assert d.e1[1, 0, 1] == 16 and d.accepted1[1, 0, 1] and 0 < d.out[0, 1, 0] < 1e-6
    lo.t[0, 1] = np.nextafter(np.float32(2), np.float32(3))             # e just above 16: dropped, the other tap alone remains
    d = up.upscale(c, lo, hi, details=True, **EXACT0)
    assert d.e1[1, 0, 1] > 16 and not d.accepted1[1, 0, 1] and d.stage[0, 1] == 1 and d.out[0, 1, 0] == 0
    assert d.stage[0, 2] == 2 and d.out[0, 2, 0] == 0                   # on pixel 1 exactly (b = 1, 0): not accepted, stage 2 finds pixel 0


def test_stage_2_takes_the_closest_valid_tap_and_the_first_one_wins_a_tie():
    """4 x 4 -> 4 x 4, output pixel (1, 1) a hit among misses except three hits in its 4 x 4 window: (0, 0) and (2, 0) at the same
    distance, (3, 2) farther.  dy runs outside dx: (0, 0) comes first."""
    c = ramp(4, 4)
    lo, hi = guides(4, 4, hit=False), guides(4, 4, hit=False)
    hi.prim[1, 1], hi.normal[1, 1], hi.t[1, 1] = 7, (0, 0, 1), 1
    for (x, y), t in (((0, 0), 2.0), ((2, 0), 2.0), ((3, 2), 4.0)):
        lo.prim[y, x], lo.normal[y, x], lo.t[y, x] = 3, (0, 0, 1), t
    d = up.upscale(c, lo, hi, details=True, **EXACT0)
    assert d.stage[1, 1] == 2 and (d.stage == 2).sum() == 4            # (and the three misses that sit on a source hit)
    assert d.out[1, 1, :3].tolist() == c[0, 0, :3].tolist()
    lo.t[0, 0] = 3                                                      # now (2, 0) is strictly closer
    assert up.upscale(c, lo, hi, **EXACT0)[1, 1, :3].tolist() == c[0, 2, :3].tolist()
    lo.normal[0, 2, 0] = np.nan                                         # a NaN distance never wins, wherever it comes
    lo.normal[0, 0, 0] = np.nan
    assert up.upscale(c, lo, hi, **EXACT0)[1, 1, :3].tolist() == c[2, 3, :3].tolist()
    lo.t[2, 3] = np.nan                                                 # every valid tap NaN: stage 3
    d = up.upscale(c, lo, hi, details=True, **EXACT0)
    assert d.stage[1, 1] == 3 and d.out[1, 1, :3].tolist() == c[1, 1, :3].tolist()


def test_stage_3_takes_the_nearest_source_pixel():
    c = ramp(3, 3)
    lo, hi = guides(3, 3, hit=False), guides(6, 6, hit=True)             # nothing comparable anywhere
    out, stage = up.upscale(c, lo, hi, stages=True, **EXACT0)
    assert (stage == 3).all()
    near = [0, 0, 1, 1, 2, 2]                                           # wx1 = 0 or 0.5: never > 0.5
    assert (out[..., :3] == c[near][:, near][..., :3]).all()
    out, stage = up.upscale(c, lo, guides(4, 4), stages=True, **EXACT0)  # fx = 0, 0.75, 1.5, 2.25
    assert (stage == 3).all() and (out[..., :3] == c[[0, 1, 1, 2]][:, [0, 1, 1, 2]][..., :3]).all()


def test_demodulation_divides_by_the_source_albedo_and_multiplies_by_the_output_albedo():
    c = ramp(2, 2) + np.float32(0.5)
    lo, hi = guides(2, 2, albedo=(0.5, 0.25, 0.001)), guides(2, 2, albedo=(2.5, 2.25, 0.002))
    out, stage = up.upscale(c, lo, hi, stages=True, **dict(up.EXACT, demodulate=1))
    assert (stage == 1).all()                                           # (the albedo term is left out of e)
    assert (out[..., 0] == c[..., 0] * 5).all() and (out[..., 1] == c[..., 1] * 9).all()
    assert (out[..., 2] == c[..., 2] / np.float32(0.01) * np.float32(0.01)).all()      # both under the floor
    out0, stage0 = up.upscale(c, lo, hi, stages=True, **EXACT0)
    assert (stage0 == 2).all()                                          # with the albedo term e = (4 + 4 + ...) * 4 > 16: no tap accepted


def test_identity_at_equal_sizes():
    for sz in ((5, 4, 5, 4), (1, 1, 1, 1)):
        c, lo, _ = up.made_up(*sz)
        out = up.upscale(c, lo, lo, demodulate=0)
        assert (out.view(np.uint32) == c.view(np.uint32)).all()


@pytest.mark.parametrize("demodulate", [0, 1])
def test_the_made_up_inputs_hold_every_case(demodulate):
    """Over the five sizes of the kernel test: all three stages, stage-1 pixels with a tap of the other class, an accepted tap at e ==
    16 and a dropped one just above, a stage-2 tie, NaN distances -- and float32 and float64 agree on every decision, so that their
    difference measures rounding alone."""
    seen = dict(stage1=0, stage2=0, stage3=0, mismatch=0, at16=0, above16=0, tie=0, nan=0)
    for sz in up.MADE_UP_SIZES:
        c, lo, hi = up.made_up(*sz)
        d = up.upscale(c, lo, hi, details=True, **dict(up.EXACT, demodulate=demodulate))
        d64 = up.upscale(c, lo, hi, details=True, dtype=np.float64, **dict(up.EXACT, demodulate=demodulate))
        assert d.out.shape == (sz[3], sz[2], 4) and np.isfinite(d.out).all() and (d.out[..., 3] == 1).all()
        assert (d.stage == d64.stage).all() and (d.accepted1 == d64.accepted1).all()
        for k in (1, 2, 3):
            seen["stage%d" % k] += int((d.stage == k).sum())
        seen["mismatch"] += int(((d.stage == 1) & (~d.valid1).any(axis=0)).sum())
        seen["at16"] += int(((d.e1 == 16) & d.accepted1).sum())
        seen["above16"] += int(((d.e1 > 16) & (d.e1 < 16.001) & d.valid1 & (d.b1 > 0)).sum())
        seen["nan"] += int((np.isnan(d.e1) & d.valid1).sum())
        emin = np.where(d.valid2 & ~np.isnan(d.e2), d.e2, np.inf).min(axis=0)
        seen["tie"] += int(((d.stage == 2) & (((d.e2 == emin) & d.valid2).sum(axis=0) >= 2)).sum())
    assert all(v > 0 for v in seen.values()), seen
