"""-m gpu: jsorb_cull_keyframes (k_kc_count, k_kc_scan_*, k_kc_scatter, k_kc_eval, k_kc_pick, k_cv_erase_dev, k_kc_apply) on the worlds of
tests/kf_culling_cases.py against the restatement there.  Every comparison is np.array_equal over ALL the arrays the call writes and all its
outputs."""
import ctypes

import numpy as np
import pytest

import kf_culling_cases as kc

pytestmark = pytest.mark.gpu
FORMS = ("async", "sync")
CAPTURE_SEED = 93                                # two culls, a row turned bad, ref_slot moved, three reparent records; another outcome the other way round


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class DeviceWorld:
    """a world's graph, table, covisibility state, views and culling state on the device"""

    def __init__(self, orb, W):
        G = W["G"]
        self.W, self.S, self.n_rows, self.pool = W, len(G["state"]), len(W["bad"]), len(G["point_pool"])
        self.graph = orb.KeyframeGraph(self.S, self.pool, 1)
        self.table = orb.MapPointTable(self.n_rows)
        self.cov = orb.Covisibility(self.S, W["C"])
        V = W["views"]
        self.views = orb.KeyframeViews(self.graph, depth=V["depth"] is not None)
        self.views.load(**{k: v for k, v in V.items() if v is not None})
        opt = lambda k: None if W[k] is None else _dev(W[k])
        self.not_erase, self.to_be_erased, self.ref_slot = opt("not_erase"), opt("to_be_erased"), opt("ref_slot")
        self.state = orb.culling_state(self.graph, self.table, self.not_erase, self.to_be_erased, self.ref_slot)
        self.load()

    def load(self):
        """everything the call writes, as the world has it, into the same device arrays"""
        W = self.W
        self.graph.load(**W["G"])
        self.graph.load(neighbours=W["cov"]["neighbours"])
        self.table.bad[:self.n_rows].copy_(_dev(W["bad"]))
        self.cov.load(**{k: W["cov"][k] for k in self.cov.ARRAYS})
        for k in ("to_be_erased", "ref_slot"):
            if W[k] is not None:
                getattr(self, k).copy_(_dev(W[k]))

    def cull(self, m, form="async", cand=None, max_cull=None, **kw):
        W = self.W
        cand = W["cand"] if cand is None else cand
        out = m.cull_keyframes(self.graph, self.table, self.cov, self.views, self.state, [int(a) for a in cand], first_slot=W["first_slot"],
                               monocular=W["monocular"], max_cull=W["max_cull"] if max_cull is None else max_cull, neighbours=self.graph.neighbours,
                               reparent_cap=W["cap"], sync=form == "sync", **kw)
        if form == "sync":
            for k in kc.OUTPUTS:
                assert np.array_equal(out[k + "_host"], out[k].cpu().numpy()), k
        stats = m.cull_keyframes_stats()
        assert [stats[k] for k in kc.COUNTS] == out["counts"].cpu().numpy().tolist()
        return self.result(out)

    def result(self, out):
        import torch
        torch.cuda.synchronize()
        g = self.graph
        res = dict(state=g.state[:self.S], registered=g.registered[:self.pool], point_pool=g.point_pool[:self.pool], parent=g.parent[:self.S],
                   bad=self.table.bad[:self.n_rows], to_be_erased=self.to_be_erased, ref_slot=self.ref_slot)
        res = {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}
        cov = self.cov.arrays()
        cov["neighbours"] = g.neighbours.cpu().numpy()
        res["cov"] = kc.cc.normalised(cov)
        res.update({k: out[k].cpu().numpy() for k in kc.OUTPUTS})
        return res


@pytest.fixture(scope="module")
def matcher(orb):
    return orb.KeyframeMatcher()


@pytest.mark.parametrize("name", list(kc.CASES))
def test_the_cases_equal_the_restatement(orb, matcher, name):
    world, expect = kc.build_case(name)
    want = kc.run_restated(world)
    for form in FORMS:
        got = DeviceWorld(orb, world).cull(matcher, form)
        kc.same(want, got, (name, form))
        kc.check_expect(got, expect, world)


def test_the_seeded_random_worlds_bit_for_bit(orb, matcher):
    n_culled = 0
    for seed in range(300):
        world = kc.random_world(seed)
        want = kc.run_restated(world)
        got = DeviceWorld(orb, world).cull(matcher)
        kc.same(want, got, world["name"])
        n_culled += int(got["counts"][2])
    assert n_culled >= 200


def test_a_map_of_many_blocks_of_rows(orb, matcher):
    # 70 000 rows: the scan of the rows' counts runs over 274 blocks, more than one pass of its top level, and the rows spread over all of them
    world = kc.random_world(18, S=300, n_rows=70000)
    want = kc.run_restated(world)
    assert want["counts"][2] >= 3 and want["counts"][5] >= 2 and want["counts"][8] >= 4
    kc.same(want, DeviceWorld(orb, world).cull(matcher), world["name"])


def test_max_cull_1_repeated_on_the_device_state_equals_one_call(orb, matcher):
    n = 0
    for seed in range(60):
        world = kc.random_world(seed)
        cand = [int(a) for a in world["cand"] if a >= 0]
        one = kc.run_restated(dict(world, max_cull=kc.MAX_CULL))
        if one["counts"][2] < 2 or len(set(cand)) != len(cand):
            continue
        n += 1
        dw, done, decision, culled = DeviceWorld(orb, world), 0, one["decision"].copy(), []
        while done < len(world["cand"]):         # the state persists on the device: the next call takes the rest of the list
            got = dw.cull(matcher, cand=world["cand"][done:], max_cull=1)
            nxt = int(got["counts"][0])
            assert nxt > 0
            decision[done:done + nxt] = got["decision"][:nxt]
            culled += [int(s) for s in got["culled_slot"] if s >= 0]
            done += nxt
        assert np.array_equal(decision, one["decision"]) and culled == [int(s) for s in one["culled_slot"] if s >= 0], world["name"]
        for k in kc.WRITTEN + ("bad", "ref_slot", "to_be_erased"):
            assert (got[k] is None and one[k] is None) or np.array_equal(got[k], one[k]), (world["name"], k)
        for k in one["cov"]:
            assert np.array_equal(got["cov"][k], one["cov"][k]), (world["name"], k)
    assert n >= 8


# ---- captured once with the scratch at its size, replayed on a fresh copy of the world with the candidates the other way round ----
def test_the_call_is_capturable(orb):
    import torch
    world = kc.random_world(CAPTURE_SEED)
    flipped = dict(world, cand=world["cand"][::-1].copy())
    want = kc.run_restated(flipped)
    assert want["counts"][2] >= 2 and want["counts"][5] >= 1 and want["decision"].tolist() != kc.run_restated(world)["decision"][::-1].tolist()
    m, dw = orb.KeyframeMatcher(), DeviceWorld(orb, world)
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    cand = _dev(world["cand"])
    args = (dw.graph, dw.table, dw.cov, dw.views, dw.state, cand)
    kw = dict(first_slot=world["first_slot"], monocular=world["monocular"], max_cull=world["max_cull"], neighbours=dw.graph.neighbours,
              reparent_cap=world["cap"])
    out = m.cull_keyframes(*args, **kw)          # the scratch and the statistics words take their size
    graph_ = torch.cuda.CUDAGraph()
    dw.load()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph_, stream=s):
        m.cull_keyframes(*args, out=out, wait=False, **kw)
    dw.load()                                    # (what the capture enqueued has not run)
    cand.copy_(cand.flip(0))                     # another order behind the same pointer
    for k in kc.OUTPUTS:
        out[k].fill_(-9)
    torch.cuda.synchronize()
    graph_.replay()
    torch.cuda.synchronize()
    kc.same(want, dw.result(out), "replayed")
    stats = m.cull_keyframes_stats()
    assert [stats[k] for k in kc.COUNTS] == want["counts"].tolist()


def test_it_follows_update_connections_on_one_matcher_in_either_order(orb):
    m = orb.KeyframeMatcher()
    world, _ = kc.build_case("a_cull_turns_rows_bad_and_pushes_the_next_over")
    want = kc.run_restated(world)
    dw = DeviceWorld(orb, world)
    kc.same(want, dw.cull(m), "before update_connections")
    m.update_connections(dw.graph, dw.table, dw.cov, [8, 9], neighbours=dw.graph.neighbours)
    assert m.update_connections_scratch()[1] == 0
    dw = DeviceWorld(orb, world)
    kc.same(want, dw.cull(m), "behind update_connections")
    assert m.update_connections_scratch()[1] == 0


def test_apply_rewrites_the_child_runs_and_the_database_is_told(orb, matcher):
    world, expect = kc.build_case("tree_weight_maximum")
    dw = DeviceWorld(orb, world)
    dw.graph = g = orb.KeyframeGraph(dw.S, dw.pool, 64)
    g.load(**world["G"])
    g.load(neighbours=world["cov"]["neighbours"])
    g.set_children(1, [4, 5, 6])
    g.set_children(2, [1])
    dw.state = orb.culling_state(g, dw.table)

    class Database:
        erased = []

        def erase(self, slot):
            self.erased.append(slot)
    out = matcher.cull_keyframes(g, dw.table, dw.cov, dw.views, dw.state, [1], first_slot=0, monocular=True, neighbours=g.neighbours, apply=True,
                                 database=Database())
    assert out["culled"] == [1] and Database.erased == [1]
    off, ln, pool = (t.cpu().numpy() for t in (g.child_off, g.child_len, g.child_pool))
    kids = lambda s: pool[off[s]:off[s] + ln[s]].tolist()
    assert kids(1) == [] and kids(2) == [5] and kids(5) == [4] and kids(4) == [6]      # (5, 2), (4, 5), (6, 4)


def test_refusals(orb, matcher):
    world, _ = kc.build_case("observations_3_4_and_two_stereo_observers")
    dw = DeviceWorld(orb, world)
    fresh = orb.KeyframeMatcher()
    with pytest.raises(orb.JsorbError, match="before"):
        fresh.cull_keyframes_stats()
    # max_cull outside [1, 16], more candidates than the build cap, no depth array for a map that is not monocular, a negative log, first_slot == S
    for kw in (dict(max_cull=0), dict(max_cull=17), dict(cand=[1] * 4097), dict(monocular=False), dict(reparent_cap=-1), dict(first_slot=dw.S)):
        kw = dict(dict(monocular=True, first_slot=0), **kw)
        with pytest.raises(orb.JsorbError):
            matcher.cull_keyframes(dw.graph, dw.table, dw.cov, dw.views, dw.state, kw.pop("cand", [1]), **kw)
    other = orb.KeyframeGraph(dw.S, dw.pool, 1)
    with pytest.raises(orb.JsorbError, match="not the graph's"):
        matcher.cull_keyframes(other, dw.table, dw.cov, dw.views, dw.state, [1], monocular=True)
    with pytest.raises(orb.JsorbError, match="max_keyframes"):
        matcher.cull_keyframes(dw.graph, dw.table, orb.Covisibility(dw.S + 1, 16), dw.views, dw.state, [1], monocular=True)
    other.registered = None
    with pytest.raises(orb.JsorbError, match="registered"):
        orb.culling_state(other, dw.table)
    # nothing was changed by the refused calls, and an empty list is a valid call
    got = dw.cull(matcher, cand=[])
    assert got["counts"].tolist() == [0] * 10 and np.array_equal(got["state"], world["G"]["state"])


def test_the_example_culls_two_and_hands_the_children_on(orb, tmp_path):
    import subprocess
    from jetson_slam_amd import build as jb
    exe = jb.build_example("keyframe_culling", str(tmp_path / "keyframe_culling"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "culled: 4 3" in r.stdout, r.stdout + r.stderr
