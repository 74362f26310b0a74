"""The evaluation loop's settled checks on the device (csrc/eval_facts.hpp; eval_chunk / eval_chunk_impl<.., FAST> in tracker_kernels.hip).

The template fact, the image fact and the pose fact select a second instantiation of the two-point loop's per-point stages that leaves
out the tests those facts settle (the tick engine's kernel on every level, the launch form's kernel on level 0).  Because the facts depend on the problem's own data alone, that instantiation must return the bits of the
general one, and a fact must never read 1 for data it does not describe:
  (a) ordinary inputs -- dsm_diag_eval_facts reports all three facts and `fast`; rs, H, b and the counts of a pose evaluation are byte for
      byte those of the same evaluation with the tracker forced general (dsm_diag_tracker_force_general): full and residual-only, the
      launch form's kernel (form 0) and the tick engine's (form 2), template sizes at one lane, the wave / chunk edges and the tail chunk;
  (b) one input spoiled at a time -- a template entry with idepth 0, 2^-70, -1 or NaN; a pixel NaN, Inf or 1e38, inside and outside the
      sampled area; a pose whose bound fails: not fast, and the bits of the forced-general run;
  (c) a fact is cleared by scaleCoarseDepthL0, by a raw plane upload and by a frame swap that brings a spoiled frame in, and set again by
      the next reference / pyramid build.
Target 96 x 64, three levels; every case takes well under a second."""
import numpy as np
import pytest

from direct_stereo_slam_amd import synth as S
from direct_stereo_slam_amd.tracker import TrackerAndScaler

pytestmark = pytest.mark.gpu

W, H, NL = 96, 64, 3
K = (80.0, 80.0, 47.5, 31.5)
SIZES = (1, 255, 256, 257, 4096, 4097)
POSE = np.array([0.004, -0.003, 0.002, 1.0, 0.02, -0.01, 0.03])
POSE[:4] /= np.linalg.norm(POSE[:4])
AFF = np.array([0.01, 1.5])
CUTOFF = 20.0
FORMS = (0, 2)  # the launch form's kernel, the tick engine's kernel
SPOT = (30, 40)  # (row, column) of a pixel the template's points sample; (0, 0) is sampled by nobody (the loop stays 2 px inside)


def base(x, y):
    return 120 + 60 * np.sin(x / 7.0) * np.cos(y / 5.0)


def image(seed):
    """one smooth pattern under seeded noise: every frame matches the template's colours up to the noise and the small motion"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    return np.clip(base(x, y) + rng.normal(scale=2.0, size=(H, W)), 0, 255).astype(np.float32)


def template(n0, seed=1):
    """per level: n points inside the level's image, positive inverse depths, colours near the image's"""
    rng = np.random.default_rng(seed)
    u, v, idp, col = [], [], [], []
    for l in range(NL):
        wl, hl = W >> l, H >> l
        n = min(n0, 300) if l else n0
        u.append(rng.uniform(4, wl - 5, n).astype(np.float32))
        v.append(rng.uniform(4, hl - 5, n).astype(np.float32))
        idp.append(rng.uniform(0.3, 2.0, n).astype(np.float32))
    if n0 > 16:  # nine far points on and around SPOT's texel (level 0): whatever the seed, some of them sample it
        g = np.array([-1.0, 0.0, 1.0], np.float32)
        u[0][:9], v[0][:9], idp[0][:9] = np.tile(SPOT[1] + g, 3) + 0.3, np.repeat(SPOT[0] + g, 3) + 0.6, 0.3
        u[0][-1], v[0][-1], idp[0][-1] = W / 2 + 0.25, H / 2 + 0.5, 1.0  # the last entry: well inside after the warp
    for l in range(NL):
        s = float(1 << l)
        col.append(base((u[l] + 0.5) * s - 0.5, (v[l] + 0.5) * s - 0.5).astype(np.float32))
    return u, v, idp, col


@pytest.fixture(scope="module")
def trk(ctx):
    t = TrackerAndScaler(ctx, W, H, NL, S.KITTI_T_STEREO, K)
    t.makeK(*K)
    yield t
    t.close()


def evaluate(t, lvl=0, pose=POSE):
    """every output of the pose evaluation in every form, full and residual-only, as bytes"""
    out = []
    for form in FORMS:
        for ro in (False, True):
            rs, Hm, b, n = t.diagEvalPose(lvl, pose, AFF, CUTOFF, form=form, residual_only=ro)
            out.append((form, ro, rs.tobytes(), Hm.tobytes(), b.tobytes(), n))
    return out


def both_ways(t, lvl=0, pose=POSE):
    """(outputs as the facts decide, outputs forced general)"""
    t.diagForceGeneral(False)
    free = evaluate(t, lvl, pose)
    t.diagForceGeneral(True)
    forced = evaluate(t, lvl, pose)
    t.diagForceGeneral(False)
    return free, forced


@pytest.mark.parametrize("n", SIZES)
def test_fast_equals_general_on_ordinary_inputs(trk, n):
    tpl = template(n, seed=n)
    if n > 16:  # negative coordinates order like the others
        tpl[0][1][20], tpl[1][1][21] = -3.5, -0.0
    trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *tpl)
    trk.upload_image(0, image(3), 1.0)
    assert trk.diagEvalFacts(0, POSE) == (1, 1, 1, 1)
    for lvl in range(NL):  # the bounds are exactly the list's: integer atomics on order-preserving keys
        bounds = trk.diagEvalFacts(lvl, POSE, with_bounds=True)[1]
        u, v, idp = (tpl[k][lvl] for k in range(3))
        assert bounds.tobytes() == np.array([u.min(), u.max(), v.min(), v.max(), idp.max()], np.float32).tobytes(), (lvl, bounds)
    free, forced = both_ways(trk)
    assert free == forced
    rs = np.frombuffer(free[0][2])
    assert free[0][5] > 0 or n == 1, "the evaluation must count points"
    assert np.isfinite(rs).all()
    trk.diagForceGeneral(True)
    assert trk.diagEvalFacts(0, POSE) == (1, 1, 1, 0)  # the facts stand, the tracker is held to the general code
    trk.diagForceGeneral(False)
    for lvl in (1, 2):  # the other levels: the tick engine's kernel has both instantiations there too, the launch form's the general one
        assert trk.diagEvalFacts(lvl, POSE)[:3] == (1, 1, 1)
        free, forced = both_ways(trk, lvl)
        assert free == forced


@pytest.mark.parametrize("bad", [0.0, 2.0 ** -70, -1.0, float("nan")])
@pytest.mark.parametrize("n", [257, 4097])
def test_spoiled_template_entry(trk, n, bad):
    tpl = template(n, seed=11)
    trk.upload_image(0, image(3), 1.0)
    trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *tpl)
    clean = evaluate(trk)
    tpl[2][0][n - 1] = bad  # the list's last entry: the tail chunk's last lane
    trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *tpl)
    tf, imf, _, fast = trk.diagEvalFacts(0, POSE)
    assert (tf, imf, fast) == (0, 1, 0)
    free, forced = both_ways(trk)
    assert free == forced
    assert free != clean  # the general code saw the entry (0, -1: not usable, :786; 2^-70: the IEEE divisions; NaN: nowhere)
    assert trk.diagEvalFacts(1, POSE)[0] == 1  # the other levels' lists are untouched


@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e38])
def test_spoiled_pixel(trk, bad, where):
    trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *template(4097, seed=12))
    im = image(4)
    trk.upload_image(0, im, 1.0)
    assert trk.diagEvalFacts(0, POSE) == (1, 1, 1, 1)
    clean = evaluate(trk)
    im = im.copy()
    im[SPOT if where == "inside" else (0, 0)] = bad
    trk.upload_image(0, im, 1.0)
    for lvl in range(NL):  # the 2x2 means carry the pixel up: 0.25 * 1e38 is still beyond 2^100
        assert trk.diagEvalFacts(lvl, POSE)[1] == 0
    assert trk.diagEvalFacts(0, POSE)[3] == 0
    free, forced = both_ways(trk)
    assert free == forced
    if where == "outside":  # nobody samples the pixel: the general code on the spoiled frame = the fast code on the clean one
        assert free == clean
    else:
        assert free != clean


def test_pose_whose_bound_fails(trk):
    trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *template(4097, seed=13))
    trk.upload_image(0, image(5), 1.0)
    for pose in ([0.0, np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4), 0.0, 0.0, 0.0],  # 90 degrees about y: pt2 changes sign inside the image
                 [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, -0.6],                               # t2 * idmax = -1.2 against M8 = 1
                 [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, float("nan")]):
        pose = np.array(pose)
        assert trk.diagEvalFacts(0, pose) == (1, 1, 0, 0)
        free, forced = both_ways(trk, 0, pose)
        assert free == forced
    assert trk.diagEvalFacts(0, POSE) == (1, 1, 1, 1)


def test_facts_are_cleared_and_set_again(ctx, trk):
    tpl = template(300, seed=14)
    trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *tpl)
    trk.upload_image(0, image(6), 1.0)
    assert trk.diagEvalFacts(0, POSE) == (1, 1, 1, 1)
    # scaleCoarseDepthL0 rewrites every inverse depth
    trk.scaleCoarseDepthL0(1.25)
    assert [trk.diagEvalFacts(l, POSE)[0] for l in range(NL)] == [0] * NL
    free, forced = both_ways(trk)
    assert free == forced
    trk.setCoarseTrackingRef(0, (0.0, 0.0), 1.0, *tpl)
    assert [trk.diagEvalFacts(l, POSE)[0] for l in range(NL)] == [1] * NL
    # a raw plane upload: nobody looked at the pixels
    planes = [trk.get_frame(0, l)[..., 0].copy() for l in range(NL)]
    trk.upload_intensity(0, planes, 1.0)
    assert [trk.diagEvalFacts(l, POSE)[1] for l in range(NL)] == [0] * NL
    trk.upload_frame(0, [trk.get_frame(0, l) for l in range(NL)], 1.0)  # (I, dx, dy) texels: no fact either
    assert [trk.diagEvalFacts(l, POSE)[1] for l in range(NL)] == [0] * NL
    ctx.upload_images([trk], [0], [image(6)])  # the batched build sets it again
    assert [trk.diagEvalFacts(l, POSE)[1] for l in range(NL)] == [1] * NL
    # a frame swap: the facts follow the buffers
    spoiled = image(7)
    spoiled[SPOT] = np.nan
    ctx.upload_images([trk], [2], [spoiled], asynchronous=True)
    ctx.upload_wait()
    assert trk.diagEvalFacts(0, POSE)[1] == 1  # the front buffer is still the good frame
    ctx.advance_frames([trk], [0])
    assert [trk.diagEvalFacts(l, POSE)[1] for l in range(NL)] == [0] * NL
    free, forced = both_ways(trk)
    assert free == forced
    ctx.upload_images([trk], [2], [image(8)], asynchronous=True)  # into what was the front buffer
    ctx.upload_wait()
    ctx.advance_frames([trk], [0])
    assert trk.diagEvalFacts(0, POSE) == (1, 1, 1, 1)
    u8 = np.clip(image(9), 0, 255).astype(np.uint8)
    ctx.upload_images([trk], [0], [u8])  # camera bytes
    assert trk.diagEvalFacts(0, POSE) == (1, 1, 1, 1)
    free, forced = both_ways(trk)
    assert free == forced
