"""The job rules of the three point calls (activation, optimisation of immature points, trace: DESIGN.md sections 12-14) are stated
once, in csrc/points_host.cpp, and used by both forms of a call.  CPU: every job of the checkers' tables of invalid calls, and a few
damaged C structures, is refused by the host form with DSM_ERR_INVALID and nothing is written.  GPU: the same job, second behind a good
job in one batched call, is refused by the device form with the same text after the call's name, nothing is written for either job, and
the context still serves a good call that equals the checker.  Every call but the last is refused before any launch."""
import numpy as np
import pytest

import _distmap_ref as DR
import _immature_ref as IR
import _trace_ref as TR

ERR_INVALID = -1
GPU_LEFT_OUT = 0  # entries of the tables that do not exist for a device job (such as a NULL target plane): none


def set_field(field, value):
    return lambda J: setattr(J, field, value)


class Activation:
    """dsm_activate_points_batch / dsm_activate_points_host on the checker's 64 x 48 case "small" """
    device_call, host_call, table_size = "dsm_activate_points_batch", "dsm_activate_points_host", 2

    def __init__(self):
        self.w, self.h, self.job, self.exp_map, self.exp_dec, _ = DR.case("small")

    def table(self):
        """the refused jobs of tests/test_distmap_ref.py and tests/test_distmap_device.py"""
        past = dict(self.job, cand_host=self.job["cand_host"].copy())
        past["cand_host"][-1] = len(self.job["kt"])
        below = dict(self.job, seed_host=self.job["seed_host"].copy())
        below["seed_host"][0] = -1
        return [("a candidate's host index past the end", past, {}), ("a seed's host index below 0", below, {})]

    def damaged(self):
        return [("kt NULL", set_field("kt", None)), ("seed_v NULL", set_field("seed_v", None)), ("decision_out NULL", set_field("decision_out", None)),
                ("n_seeds -1", set_field("n_seeds", -1)), ("n_cand -1", set_field("n_cand", -1)), ("n_hosts -1", set_field("n_hosts", -1))]

    def batch(self, jobs):
        from direct_stereo_slam_amd import distmap

        b = distmap.ActivationBatch(jobs)
        for dec, nact, _ in b.outs:
            dec[:], nact[:] = 77, -5
        b.host_map = np.full((self.h >> 1, self.w >> 1), -3.0, np.float32)
        return b

    def outputs(self, b):
        maps = [j["map"].get() for j in b.jobs if j.get("map") is not None]
        return [a for dec, nact, _ in b.outs for a in (dec, nact)] + [b.host_map] + maps

    def open(self, ctx):
        from direct_stereo_slam_amd import distmap

        self.maps = [distmap.DistanceMap(ctx, self.w, self.h) for _ in range(2)]

    def close(self):
        for m in self.maps:
            m.close()

    def on_device(self, job, k):
        return dict(job, map=self.maps[k])

    def run_host(self, b, kw):
        b.run_host(self.w, self.h, 0, b.host_map)

    def run_device(self, ctx, b, kw):
        b.run(ctx)

    def good_call_equals_checker(self, ctx):
        from direct_stereo_slam_amd import distmap

        res = distmap.activate_points_batch(ctx, [self.on_device(self.job, 0)])[0]
        assert np.array_equal(self.maps[0].get(), self.exp_map) and np.array_equal(res["decisions"], self.exp_dec)


class Immature:
    """dsm_optimize_immature_points_batch / _host on the checker's 96 x 64 case "two_frames" """
    device_call, host_call, table_size = "dsm_optimize_immature_points_batch", "dsm_optimize_immature_points_host", 6

    def __init__(self):
        self.job, self.frames, self.exp, _ = IR.case("two_frames")

    def table(self):
        return IR.invalid_jobs(self.job)

    def damaged(self):
        return [("n_frames 0", set_field("n_frames", 0)), ("n_frames 10", set_field("n_frames", 10)), ("n_pts -1", set_field("n_pts", -1)),
                ("pre_t NULL", set_field("pre_t", None)), ("weights NULL", set_field("weights", None)), ("res_state NULL", set_field("res_state", None))]

    def batch(self, jobs):
        from direct_stereo_slam_amd import immature

        return immature.ImmatureBatch(jobs)

    def outputs(self, b):
        return [a for out, _ in b.outs for a in out.values()]

    def open(self, ctx):
        from direct_stereo_slam_amd import immature

        self.win = immature.KeyframeWindow(ctx, IR.W, IR.H, len(self.frames))
        for fid, img in zip(self.job["frame_ids"], self.frames):
            self.win.put_host(int(fid), img)

    def close(self):
        self.win.close()

    def on_device(self, job, k):
        return dict(job, window=self.win)

    def run_host(self, b, kw):
        b.run_host(IR.W, IR.H, 0, self.frames, **kw)

    def run_device(self, ctx, b, kw):
        b.run(ctx, **kw)

    def good_call_equals_checker(self, ctx):
        from direct_stereo_slam_amd import immature

        IR.assert_equal(immature.optimize_immature_points_batch(ctx, [self.on_device(self.job, 0)])[0], self.exp)


class Trace:
    """dsm_trace_points_batch / _host on the first eight points of the checker's 160 x 64 case "no_gn" """
    device_call, host_call, table_size = "dsm_trace_points_batch", "dsm_trace_points_host", 18

    def __init__(self):
        job, self.target, exp, self.params = TR.case("no_gn")
        idx = np.arange(8)
        self.job, self.exp = TR.subset(job, idx), TR.subset_result(exp, idx)

    def table(self):
        return TR.invalid_calls(self.job)

    def damaged(self):
        return [("n_hosts -1", set_field("n_hosts", -1)), ("n_pts -1", set_field("n_pts", -1)), ("aff NULL", set_field("aff", None)),
                ("grad_h NULL", set_field("grad_h", None)), ("trace_uv NULL", set_field("trace_uv", None))]

    def batch(self, jobs):
        from direct_stereo_slam_amd import trace

        return trace.TraceBatch(jobs)

    def outputs(self, b):
        return [a for st, _ in b.state for a in st.values()]

    def open(self, ctx):
        from direct_stereo_slam_amd import immature

        self.win = immature.KeyframeWindow(ctx, TR.W, TR.H, 1)
        self.win.put_host(0, self.target)

    def close(self):
        self.win.close()

    def on_device(self, job, k):
        return dict(job, target=self.win, target_frame_id=0)

    def run_host(self, b, kw):
        from direct_stereo_slam_amd import trace

        b.run_host(TR.W, TR.H, 0, self.target, trace.params(**kw))

    def run_device(self, ctx, b, kw):
        from direct_stereo_slam_amd import trace

        b.run(ctx, trace.params(**kw))

    def good_call_equals_checker(self, ctx):
        from direct_stereo_slam_amd import trace

        TR.assert_equal(trace.trace_points_batch(ctx, [self.on_device(self.job, 0)], **self.params)[0], self.exp)


CALLS = [Activation, Immature, Trace]


def entries(call):
    """(what, job, keyword arguments, change to the C structure or None): the checker's table, then the damaged structures"""
    return [(what, job, kw, None) for what, job, kw in call.table()] + [(what, call.job, {}, change) for what, change in call.damaged()]


def refused(run, b, job_index, change, outputs, name):
    """the text after "<name>: " of the DSM_ERR_INVALID that run() must raise; no output of the batch changes"""
    from direct_stereo_slam_amd._lib import DsmError

    if change:
        change(b.arr[job_index])
    before = [a.copy() for a in outputs(b)]
    with pytest.raises(DsmError) as e:
        run()
    head = f"dsm error {ERR_INVALID}: {name}: "
    assert str(e.value).startswith(head), str(e.value)
    assert all(a.tobytes() == bef.tobytes() for a, bef in zip(outputs(b), before))
    return str(e.value)[len(head):]


def host_refusal(call, job, kw, change):
    b = call.batch([job])
    b.jobs = [job]
    return refused(lambda: call.run_host(b, kw), b, 0, change, call.outputs, call.host_call)


@pytest.mark.parametrize("make", CALLS)
def test_host_form_refuses_every_entry_and_writes_nothing(built, make):
    call = make()
    assert len(call.table()) >= call.table_size  # every entry of the checker's table is covered: the loop below takes them all
    texts = {what: host_refusal(call, job, kw, change) for what, job, kw, change in entries(call)}
    assert len(texts) == len(call.table()) + len(call.damaged()) and all(texts.values())
    assert len(set(texts.values())) >= 3  # the refusals name their rule


@pytest.mark.gpu
@pytest.mark.parametrize("make", CALLS)
def test_device_form_refuses_the_same_jobs_with_the_same_words(ctx, make):
    call = make()
    call.open(ctx)
    left_out = 0
    for what, job, kw, change in entries(call):
        jobs = [call.on_device(call.job, 0), call.on_device(job, 1)]
        b = call.batch(jobs)
        b.jobs = jobs
        on_device = refused(lambda: call.run_device(ctx, b, kw), b, 1, change, call.outputs, call.device_call)
        assert on_device == host_refusal(call, job, kw, change), what
    assert left_out == GPU_LEFT_OUT
    call.good_call_equals_checker(ctx)
    call.close()


@pytest.mark.gpu
def test_distmaps_make_shares_the_seed_rules(ctx):
    """dsm_distmaps_make reads no candidate: a bad seed is refused in the host form's words, a bad candidate is not looked at"""
    from direct_stereo_slam_amd import distmap

    call = Activation()
    call.open(ctx)
    (_, bad_cand, _), (_, bad_seed, _) = call.table()
    jobs = [call.on_device(call.job, 0), call.on_device(bad_seed, 1)]
    b = call.batch(jobs)
    b.jobs = jobs
    assert refused(lambda: b.make(ctx), b, 1, None, call.outputs, "dsm_distmaps_make") == host_refusal(call, bad_seed, {}, None)
    distmap.make_distance_maps(ctx, [call.on_device(bad_cand, 0)])
    assert np.array_equal(call.maps[0].get(), DR.case("small")[5]["initial_map"])
    call.close()
