"""MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:273-338 of the reference) on the host, twice:
  reference_point / transcription  the sequential code, line by line, with the sort and the 0.5*(N-1) index as written;
  restatement                      the method of k_distinct.hip in numpy - the rank by counting over nine halving steps, the winner as the minimum
                                   of the key (median, i) - over a whole call, every output array and statistics word of
                                   jsorb_distinctive_descriptors (include/jsorb.h) for given build caps.
A WORLD is what a test and the reference driver (tools/ref_mappoint/) share: keyframes in ONE array (so pointer order is array order), each with a
descriptor matrix and a bad flag, and per point the raw observations (keyframe, keypoint), ascending keyframes, the bad ones INCLUDED; csr() leaves
them out as the caller of the device call does.  Everything is integer-exact."""
import numpy as np

SHIPPED = (16, 64, 1024)                         # DD_GROUP_LANES, DD_WAVE_LANES, DD_LDS_DESC of k_distinct.hip
TINY = (4, 8, 16)                                # the tiny_distinct build (jetson_slam_amd/build.py VARIANTS)
BLOCK_SEEDS = (11, 12)
# the N every block holds: each tier boundary and one above it for both builds, the small cases, even and odd
FORCED_N = (0, 1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65, 1024, 1025)
INT_MAX = 2 ** 31 - 1


def as_ints(D):
    """the rows of a uint8[N, 32] matrix as Python ints (a popcount of an xor each distance)"""
    return [int.from_bytes(bytes(r), "little") for r in np.asarray(D, np.uint8).reshape(-1, 32)]


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance (ORBmatcher.cpp:1653-1671): the bit count of the xor over eight 32-bit words"""
    return bin(a ^ b).count("1")


def transcription(D):
    """:304-332 for the descriptors D uint8[N, 32], N >= 1 -> (BestIdx, BestMedian)"""
    v = as_ints(D)
    N = len(v)                                                       # :304
    dist = [[0.0] * N for _ in range(N)]                             # :306 float Distances[N][N]
    for i in range(N):                                               # :307
        dist[i][i] = 0.0                                             # :309
        for j in range(i + 1, N):                                    # :310
            distij = descriptor_distance(v[i], v[j])                 # :312
            dist[i][j] = float(distij)                               # :313
            dist[j][i] = float(distij)                               # :314
    best_median, best_idx = INT_MAX, 0                               # :319-320
    for i in range(N):                                               # :321
        vdists = [int(x) for x in dist[i]]                           # :323 vector<int> from the floats
        vdists.sort()                                                # :324
        median = vdists[int(0.5 * (N - 1))]                          # :325
        if median < best_median:                                     # :327
            best_median, best_idx = median, i                        # :329-330
    return best_idx, best_median


def reference_point(observations, old):
    """:273-337 for one good point: observations = [(descriptor uint8[32], keyframe is bad)] in map order, old = mDescriptor before the call.
    -> (mDescriptor after, BestIdx among the kept observations or -1, BestMedian or -1)"""
    if not observations:                                             # :287
        return old, -1, -1
    kept = [d for d, bad in observations if not bad]                 # :292-298
    if not kept:                                                     # :300
        return old, -1, -1
    bi, bm = transcription(np.stack(kept))
    return np.array(kept[bi], np.uint8), bi, bm                      # :336


# ---- the kernels' method ----
_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint16)


def pairwise(D):
    """int32[N, N] Hamming distances of the rows of D uint8[N, 32]"""
    w = np.ascontiguousarray(D, np.uint8).reshape(-1, 32).view(np.uint16)
    return _POP16[w[:, None, :] ^ w[None, :, :]].sum(axis=2, dtype=np.int32)


def rank_by_counting(d, need):
    """per row of d (values in [0, 256]) the smallest v with `need` entries <= v: nine halving steps over [0, 256]"""
    lo, hi = np.zeros(len(d), np.int32), np.full(len(d), 256, np.int32)
    for _ in range(9):
        mid = (lo + hi) >> 1
        ok = (d <= mid[:, None]).sum(axis=1) >= need
        hi = np.where(ok, mid, hi)
        lo = np.where(ok, lo, mid + 1)
    return lo


def point_by_keys(D):
    """-> (BestIdx, BestMedian) as the kernels find them: the minimum of median << 32 | i"""
    N = len(D)
    med = rank_by_counting(pairwise(D), (N - 1) // 2 + 1)
    key = int((med.astype(np.int64) << 32 | np.arange(N, dtype=np.int64)).min())
    return key & 0xffffffff, key >> 32


def restatement(obs_start, obs_row, kf_desc, out_row=None, desc_out=None, want_changed=False, n_obs=None, n_rows=None, n_out_rows=None, caps=SHIPPED):
    """the device call on the host -> dict(best_obs, best_median, desc_out (a copy, or None), changed (or None), stats (the eight words))"""
    obs_start, obs_row = np.asarray(obs_start, np.int64), np.asarray(obs_row, np.int64)
    kf_desc = np.asarray(kf_desc, np.uint8).reshape(-1, 32)
    n = len(obs_start) - 1
    n_obs = len(obs_row) if n_obs is None else n_obs
    n_rows = len(kf_desc) if n_rows is None else n_rows
    out = None if desc_out is None else np.array(desc_out, np.uint8).reshape(-1, 32)
    n_out_rows = (0 if out is None else len(out)) if n_out_rows is None else n_out_rows
    best_obs, best_median = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    changed = np.zeros(n, np.uint8) if want_changed else None
    st = [0] * 8
    for p in range(n):
        s, e = int(obs_start[p]), int(obs_start[p + 1])
        r = -1 if out is None else p if out_row is None else int(out_row[p])
        if s < 0 or s > n_obs or e < 0 or e > n_obs or e < s or (out is not None and not 0 <= r < n_out_rows):
            st[5] += 1
            continue
        N = e - s
        if N == 0:
            st[4] += 1
            continue
        st[0 if N <= caps[0] else 1 if N <= caps[1] else 2] += 1
        st[3] += N > caps[1] and N > caps[2]
        st[7] = max(st[7], N)
        rows = obs_row[s:e]
        if ((rows < 0) | (rows >= n_rows)).any():
            st[5] += 1
            continue
        bi, bm = point_by_keys(kf_desc[rows])
        best_obs[p], best_median[p] = bi, bm
        if out is not None:
            diff = not np.array_equal(out[r], kf_desc[rows[bi]])
            out[r] = kf_desc[rows[bi]]
            st[6] += diff
            if want_changed:
                changed[p] = diff
    return dict(best_obs=best_obs, best_median=best_median, desc_out=out, changed=changed, stats=tuple(int(x) for x in st))


# ---- worlds ----
def csr(w):
    """the device call's observations of a world: (obs_start int32[P + 1], obs_row int32[.]) with the bad keyframes left out, order kept"""
    keep = w["kf_bad"][w["obs_kf"]] == 0
    start = np.concatenate([[0], np.cumsum(keep)])[w["obs_start"]].astype(np.int32)
    return start, (w["kf_start"][w["obs_kf"]] + w["obs_idx"])[keep].astype(np.int32)


def world_reference(w, old=None):
    """reference_point over every point of a world -> (descriptors uint8[P, 32] after the call, best_obs, best_median); old: uint8[P, 32] or
    None (zeros)"""
    P = len(w["obs_start"]) - 1
    old = np.zeros((P, 32), np.uint8) if old is None else np.asarray(old, np.uint8)
    out, bo, bm = old.copy(), np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    for p in range(P):
        o = range(w["obs_start"][p], w["obs_start"][p + 1])
        obs = [(w["kf_desc"][w["kf_start"][w["obs_kf"][i]] + w["obs_idx"][i]], bool(w["kf_bad"][w["obs_kf"][i]])) for i in o]
        out[p], bo[p], bm[p] = reference_point(obs, old[p])
    return out, bo, bm


def clustered(rng, n, n_bases=6, max_flips=3):
    """n descriptors a few bit flips around a handful of bases: medians tie often (uniformly random descriptors almost never do)"""
    bases = rng.integers(0, 256, (n_bases, 32), dtype=np.uint8)
    d = bases[rng.integers(0, n_bases, n)].copy()
    for i in range(n):
        for b in rng.integers(0, 256, rng.integers(0, max_flips + 1)):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def block(seed, n_extra=48, n_kf=1100, per_kf=3, forced=FORCED_N):
    """a random world: n_kf keyframes of per_kf keypoints (a twentieth of them bad), one point per forced N and n_extra points with N in [2, 20];
    N counts the GOOD observations, and every point with N > 0 sees one or two bad keyframes on top where the draw allows"""
    rng = np.random.default_rng(seed)
    kf_bad = (rng.random(n_kf) < 0.05).astype(np.uint8)
    good, bad = np.nonzero(kf_bad == 0)[0], np.nonzero(kf_bad)[0]
    assert len(good) >= max(forced)
    ns = list(forced) + [int(x) for x in rng.integers(2, 21, n_extra)]
    order = rng.permutation(len(ns))
    obs_start, obs_kf = [0], []
    for k in order:
        n_bad = int(rng.integers(0, 3)) if ns[k] or rng.random() < 0.5 else 0
        kfs = np.sort(np.concatenate([rng.choice(good, ns[k], replace=False), rng.choice(bad, n_bad, replace=False)]))
        obs_kf += [int(x) for x in kfs]
        obs_start.append(len(obs_kf))
    obs_kf = np.array(obs_kf, np.int32)
    return dict(kf_start=(np.arange(n_kf + 1) * per_kf).astype(np.int32), kf_desc=clustered(rng, n_kf * per_kf), kf_bad=kf_bad,
                obs_start=np.array(obs_start, np.int32), obs_kf=obs_kf, obs_idx=rng.integers(0, per_kf, len(obs_kf)).astype(np.int32))


def coverage(w, bo=None, caps=(SHIPPED, TINY)):
    """the counters every random block must show non-zero"""
    start, row = csr(w)
    N = np.diff(start)
    if bo is None:
        bo = world_reference(w)[1]
    tied = 0
    for p in np.nonzero(N > 1)[0]:
        D = w["kf_desc"][row[start[p]:start[p + 1]]]
        med = rank_by_counting(pairwise(D), (len(D) - 1) // 2 + 1)
        tied += int((med == med.min()).sum() > 1)
    c = dict(tied=tied, not_first=int((bo > 0).sum()), even=int(((N > 0) & (N % 2 == 0)).sum()), odd=int((N % 2 == 1).sum()), empty=int((N == 0).sum()),
             bad_skipped=int((w["kf_bad"][w["obs_kf"]] != 0).sum()))
    for cap in caps:
        for b in cap:
            c["n_%d" % b], c["n_%d" % (b + 1)] = int((N == b).sum()), int((N == b + 1).sum())
    return c


# ---- constructed cases: one decision each ----
def _d(*bits):
    """a descriptor with the given bits set"""
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b >> 3] |= 1 << (b & 7)
    return d


def _far(k):
    """descriptors pairwise 2 k apart and k from zero: disjoint runs of k bits"""
    return lambda i: _d(*range(i * k, (i + 1) * k))


def constructed():
    """name -> (observations [(descriptor, bad)], BestIdx among the kept ones, BestMedian) (-1, -1: mDescriptor stays)"""
    A, B, C, E = _d(), _d(0), _d(0, 1, 2), _d(0, 1, 2, 3, 4, 5)
    ones = np.full(32, 255, np.uint8)
    good = lambda *ds: [(np.array(d, np.uint8), False) for d in ds]
    c = {}
    c["n0"] = ([], -1, -1)
    c["n0_all_bad"] = ([(B, True), (C, True)], -1, -1)
    c["n1"] = (good(E), 0, 0)
    c["n2"] = (good(E, A), 0, 0)                                     # both medians are the self-distance: index 0 whatever the descriptors
    c["n2_swapped"] = (good(A, E), 0, 0)
    # N = 3: the median is the SMALLER real distance.  A-B 1, A-E 6, B-E 5: rows (0,1,6) (0,1,5) (0,5,6) -> medians 1, 1, 5: the first of the tie
    c["n3"] = (good(A, B, E), 0, 1)
    c["n3_upper_would_differ"] = (good(E, A, B), 1, 1)               # medians 5, 1, 1; the larger distances (6, 6, 5) would pick index 2
    # even N = 4, index 1 = (N-1)/2: rows of A, B, C, F.  lower middles decide, upper middles would pick another row
    F = _d(*range(100, 110))
    # A-B 1, A-C 3, A-F 10, B-C 2, B-F 11, C-F 13: sorted rows A (0,1,3,10) B (0,1,2,11) C (0,2,3,13) F (0,10,11,13)
    # lower middles 1, 1, 2, 10 -> A (first); upper middles 3, 2, 3, 11 -> B
    c["n4_lower_middle"] = (good(A, B, C, F), 0, 1)
    c["n4_lower_middle_only"] = (good(C, A, B, F), 1, 1)             # lower middles 2, 1, 1, 10 -> index 1; upper middles 3, 3, 2, 11 -> index 2
    # a tie on the best median: the FIRST row wins, and with the two swapped the other descriptor comes out
    G, H = _d(200), _d(201)                                          # G-H 2; both 1 from A
    c["tie_first"] = (good(G, H, A, A), 2, 0)                        # rows G (0,1,1,2) H (0,1,1,2) A (0,0,1,1) A: medians 1, 1, 0, 0 -> index 2
    c["tie_pair"] = (good(G, H, _d(200, 201, 202)), 0, 2)            # G-H 2, G-X 2, H-X 2: medians 2, 2, 2 -> index 0, which is G
    c["tie_pair_swapped"] = (good(H, G, _d(200, 201, 202)), 0, 2)    # the same point, two observations swapped: index 0 is now H
    # no tie on the best median: any order gives the same bytes.  Medians A 1, B 2, _d(1) 2, f(0) 19, f(1) 21 -> A wherever it stands
    f = _far(20)
    c["permute_a"] = (good(f(0), B, A, _d(1), f(1)), None, None)
    c["permute_b"] = (good(_d(1), f(1), f(0), A, B), None, None)
    c["duplicated_row"] = (good(C, C, E, A), 0, 0)                   # rows C (0,0,3,3): median 0
    c["all_identical"] = (good(E, E, E, E, E), 0, 0)
    c["complements"] = (good(A, ones, ones), 1, 0)                   # distances 0 and 256: rows A (0,256,256) -> 256, ones (0,0,256) -> 0
    c["complements_256"] = (good(A, ones), 0, 0)
    c["max_median"] = (good(A, ones, A, ones), 0, 0)
    c["bad_left_out"] = ([(E, False), (F, True), (A, False), (B, False)], 1, 1)       # kept E, A, B: medians 5, 1, 1 -> A, index 1 of the kept
    c["bad_changes_winner"] = ([(E, False), (A, True), (B, False), (C, False)], 1, 2)  # kept E, B, C: medians 3, 2, 2 -> B; with A counted in, A would win
    return c


def constructed_world(cases=None):
    """the constructed cases as ONE world: point p observes the keyframes 0 .. len - 1 at keypoint p; a keyframe is bad for every point, so the
    cases with bad observations get keyframes of their own behind the shared good ones"""
    cases = constructed() if cases is None else cases
    names = list(cases)
    P = len(names)
    n_good = max(len(cases[n][0]) for n in names)
    slots = []                                   # per point the keyframe of each observation: ascending
    n_kf = n_good
    for n in names:
        obs = cases[n][0]
        if any(bad for _, bad in obs):
            # the point's bad observations need bad keyframes BETWEEN its good ones: a run of fresh keyframes, all past the shared ones
            ks = list(range(n_kf, n_kf + len(obs)))
            n_kf += len(obs)
        else:
            ks = list(range(len(obs)))
        slots.append(ks)
    kf_bad = np.zeros(n_kf, np.uint8)
    kf_desc = np.zeros((n_kf * P, 32), np.uint8)
    obs_start, obs_kf, obs_idx = [0], [], []
    for p, n in enumerate(names):
        for (d, bad), k in zip(cases[n][0], slots[p]):
            kf_desc[k * P + p] = d
            kf_bad[k] |= bad
            obs_kf.append(k)
            obs_idx.append(p)
        obs_start.append(len(obs_kf))
    return names, dict(kf_start=(np.arange(n_kf + 1) * P).astype(np.int32), kf_desc=kf_desc, kf_bad=kf_bad, obs_start=np.array(obs_start, np.int32),
                       obs_kf=np.array(obs_kf, np.int32), obs_idx=np.array(obs_idx, np.int32))


# ---- mutants: each must fail a case of the reference's recorded outputs (tests/test_ref_mappoint.py) ----
MUTANTS = ("upper_middle", "no_self_distance", "less_equal", "last_of_ties", "mean", "descending_sort")


def mutant_point(D, mutant):
    """transcription() with one decision changed -> BestIdx"""
    d = pairwise(D)
    N = len(d)
    best, best_idx = None, 0
    order = range(N - 1, -1, -1) if mutant == "last_of_ties" else range(N)
    for i in order:
        row = sorted(int(x) for x in d[i])
        if mutant == "upper_middle":
            m = row[N // 2]
        elif mutant == "no_self_distance":
            rest = sorted(int(x) for j, x in enumerate(d[i]) if j != i)
            m = rest[int(0.5 * (N - 2))] if rest else 0
        elif mutant == "mean":
            m = sum(row)                                             # the mean's order is the sum's
        elif mutant == "descending_sort":
            m = row[::-1][int(0.5 * (N - 1))]
        else:
            m = row[int(0.5 * (N - 1))]
        if best is None or (m <= best if mutant == "less_equal" else m < best):
            best, best_idx = m, i
    return best_idx


# ---- the reference's own MapPoint.cpp (authoring machines: tools/ref_mappoint/, built into oracle/_ref/, which git ignores) ----
GOLDEN = "ref_matcher_mappoint_distinctive"        # (the ref_matcher_ prefix: the fixture tests that walk tests/golden/*.npz leave such files to their own tests)


def _root():
    import os
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def driver_path():
    import os
    return os.path.join(_root(), "oracle", "_ref", "ref_mappoint_driver")


def reference_tree():
    """the reference tree, or None where it is absent"""
    import os
    ref = os.environ.get("JSORB_REFERENCE", "/root/reference")
    return ref if os.path.exists(os.path.join(ref, "src", "MapPoint.cpp")) else None


def build_driver(reference):
    """the reference's src/MapPoint.cpp, src/ORBmatcher.cpp (DescriptorDistance) and DBoW2's FeatureVector.cpp, unmodified, with tools/ref_mappoint's
    stand-ins force-included so that their guards shut out the reference's KeyFrame.h / Frame.h / Map.h; a stand-alone program whose unused
    sections (the matchers, whose KeyFrame / Frame members nobody defines) are discarded at link time"""
    import os
    import subprocess
    shadow = os.path.join(_root(), "tools", "ref_mappoint")
    os.makedirs(os.path.dirname(driver_path()), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-fno-fast-math", "-w", "-ffunction-sections", "-fdata-sections", "-I" + shadow,
           "-I" + os.path.join(reference, "include"), "-I" + reference]
    for h in ("KeyFrame.h", "Frame.h", "Map.h"):
        cmd += ["-include", os.path.join(shadow, h)]
    cmd += ["-o", driver_path(), os.path.join(shadow, "driver.cpp"), os.path.join(reference, "src", "MapPoint.cpp"), os.path.join(reference, "src", "ORBmatcher.cpp"),
            os.path.join(reference, "Thirdparty", "DBoW2", "DBoW2", "FeatureVector.cpp"), "-Wl,--gc-sections", "-lpthread"]
    subprocess.check_call(cmd)
    return driver_path()


def run_driver(w, workdir):
    """a world through the reference -> (has uint8[P]: GetDescriptor() is not empty, descriptors uint8[P, 32])"""
    import os
    import subprocess
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()
    P = len(w["obs_start"]) - 1
    src, dst = os.path.join(workdir, "world.bin"), os.path.join(workdir, "out.bin")
    with open(src, "wb") as f:
        f.write(i32([len(w["kf_bad"]), len(w["kf_desc"]), P, len(w["obs_kf"])]) + i32(w["kf_start"]) + i32(w["kf_bad"]) + i32(w["obs_start"]) +
                i32(w["obs_kf"]) + i32(w["obs_idx"]) + np.ascontiguousarray(w["kf_desc"], np.uint8).tobytes())
    subprocess.check_call([driver_path(), src, dst], timeout=120)
    out = np.fromfile(dst, np.uint8).reshape(P, 33)
    return out[:, 0].copy(), out[:, 1:].copy()


def fixture_worlds():
    """name -> world: what tests/golden/ref_matcher_mappoint_distinctive.npz holds, inputs as generated here"""
    worlds = {"constructed": constructed_world()[1]}
    for seed in BLOCK_SEEDS:
        worlds["random_%d" % seed] = block(seed)
    return worlds


def golden_path():
    import os
    return os.path.join(_root(), "tests", "golden", GOLDEN + ".npz")


def save_golden(worlds):
    """name -> flat dict of arrays, as an npz with a fixed member order and no timestamps: regenerating gives the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(golden_path(), "w", zipfile.ZIP_DEFLATED) as z:
        for name in worlds:
            for key in sorted(worlds[name]):
                buf = io.BytesIO()
                np.save(buf, np.ascontiguousarray(worlds[name][key]), allow_pickle=False)
                z.writestr(zipfile.ZipInfo("%s.%s.npy" % (name, key), date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    return golden_path()


def load_golden():
    """name -> dict of arrays, in the file's order"""
    out = {}
    with np.load(golden_path()) as z:
        for member in z.files:
            name, key = member.split(".", 1)
            out.setdefault(name, {})[key] = z[member]
    return out
