"""CPU: the hostile plane inputs (tests/hard_planes.py) can do what they are for.  The restatement (tests/planes_restate.py) reproduces
every array the reference recorded on trimmed subsets of them (tests/golden/planes_hostile.npz, tools/plane_fixture/gen.py);
`offset_variants(...)["plain"]` is the restatement bit for bit; every family holds the witnesses it is meant to hold, so a kernel
with contracted, reordered or precomputed arithmetic gives other counts on it; the closed-form counts of the `exact` family are the
restatement's; the subnormal block shows a flush to zero; the tie clouds have their index properties."""
import numpy as np
import pytest

from conftest import load_golden
import hard_planes as H
import planes_restate as R

F = np.float32


@pytest.fixture(scope="module")
def golden():
    return load_golden("planes_hostile.npz")


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in H.vote_cases()}


@pytest.fixture(scope="module")
def witnesses(cases):
    return {name: H.vote_witnesses(c) for name, c in cases.items()}


def rounds_of(g, prefix):
    return [{k: g[f"{prefix}r{r}_{k}"] for k in ("idx", "valid", "counts", "best", "mask_before", "mask_after")} for r in range(int(g[prefix + "n_rounds"]))]


def check_detection(g, prefix):
    fm, wm = R.candidate_masks(g[prefix + "nor"], g[prefix + "dot_threshold"])
    assert (fm == g[prefix + "floor_mask"]).all() and (wm == g[prefix + "wall_mask"]).all()
    got = R.detect(g[prefix + "pos"], g[prefix + "nor"], g[prefix + "dot_threshold"], g[prefix + "dist_threshold"], int(g[prefix + "count_threshold"]))
    want = rounds_of(g, prefix)
    assert len(got["rounds"]) == len(want)
    for k, (a, b) in enumerate(zip(got["rounds"], want)):
        assert (a["idx"] == b["idx"]).all() and (a["valid"] == b["valid"]).all() and a["best"] == int(b["best"]), (prefix, k)
        assert (a["counts"] == np.where(b["valid"] != 0, b["counts"], 0)).all(), (prefix, k)
        assert (R.votes(g[prefix + "pos"], b["mask_before"], a["center"], a["normal"], g[prefix + "dist_threshold"]) == b["counts"]).all(), (prefix, k)
        assert (a["mask_before"] == b["mask_before"]).all() and (a["mask_after"] == b["mask_after"]).all(), (prefix, k)
    assert R.same_bits(got["centers"], g[prefix + "centers"]) and R.same_bits(got["normals"], g[prefix + "normals"])
    assert (got["n_inliers"] == g[prefix + "n_inliers"]).all() and got["n_floors"] == int(g[prefix + "n_floors"]) and got["n_walls"] == int(g[prefix + "n_walls"])
    return got


def test_fixture_holds_the_generators_subsets(golden, cases):
    assert golden["vote_cases"].tolist() == list(cases)
    for name, case in cases.items():
        c = H.trimmed(case)
        for k in ("pos", "center", "normal"):
            assert R.same_bits(golden[f"votes_{name}_{k}"], c[k]), (name, k)
        assert 500 <= len(c["pos"]) <= 512 and c["center"].shape == (64, 3)
    for name, family in H.GATHER_FAMILIES.items():
        c = family(257)
        assert R.same_bits(golden[f"gather_{name}_pos"], c["pos"]) and R.same_bits(golden[f"gather_{name}_nor"], c["nor"]), name
        for k, v in c["models"].items():
            assert golden[f"gather_{name}_model_{k}"].tobytes() == v.tobytes(), (name, k)


def test_restatement_reproduces_the_recorded_votes_and_removals(golden, cases):
    for name, case in cases.items():
        c, p = H.trimmed(case), f"votes_{name}_"
        for mname, m in H.vote_masks(c).items():
            got = R.votes(c["pos"], m, c["center"], c["normal"], c["dist_threshold"])
            assert (got == golden[p + "counts_" + mname]).all(), (name, mname, np.flatnonzero(got != golden[p + "counts_" + mname])[:5])
        full = np.ones(len(c["pos"]), np.uint8)
        for j in range(8):
            assert (R.remove(c["pos"], full, c["center"][j], c["normal"][j], c["dist_threshold"]) == golden[p + "removed"][j]).all(), (name, j)
    # the recordings themselves hold what the families are for
    assert golden["votes_special_counts_all"][1] == np.isfinite(golden["votes_special_pos"]).all(axis=1).sum()          # the zero normal
    assert golden["votes_special_counts_all"][0] == 0 and golden["votes_special_counts_all"][2] == 0 and golden["votes_special_counts_all"][3] == 0
    assert golden["votes_special_subnormal_counts_all"].min() > 0


def test_restatement_reproduces_the_recorded_gather_and_relabel(golden):
    for name, family in H.GATHER_FAMILIES.items():
        c, p = family(257), f"gather_{name}_"
        M = c["models"]
        for pname, dot, dist, cv, ce in (("plain", 0.8, 0.05, False, False), ("checked", 0.0, 0.05, True, True)):
            got = R.gather(c["pos"], c["nor"], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], dot, dist, cv, ce)
            o = golden[p + pname + "_offsets"]
            for m in range(len(got)):
                assert (got[m] == golden[p + pname + "_index"][o[m]:o[m + 1]]).all() and len(got[m]) == o[m + 1] - o[m], (name, pname, m)
        assert (c["cls"] == golden[p + "class_before"]).all() and (c["inst"] == golden[p + "instance_before"]).all()
        cls, inst = R.relabel(c["pos"], c["nor"], M["center"], M["normal"], M["axes"], M["extends"], M["valid"], M["up_dot"], *c["ids"], c["cls"], c["inst"])
        assert (cls == golden[p + "class_after"]).all() and (inst == golden[p + "instance_after"]).all(), name


def test_restatement_reproduces_the_probe_room_and_the_tie_cloud(golden):
    room = H.room_with_probes()
    assert R.same_bits(room["pos"], golden["room_pos"]) and R.same_bits(room["nor"], golden["room_nor"])
    assert (room["band"] == golden["room_band"]).all() and (room["probes"] == golden["room_probes"]).all()
    got = check_detection(golden, "room_")
    assert got["n_floors"] == 1 and got["n_walls"] >= 2 and got["rounds"][1]["best"] == room["best"]
    # the probes: every edge of both masks, on both sides
    fm, wm = golden["room_floor_mask"][room["probes"]], golden["room_wall_mask"][room["probes"]]
    nor = room["nor"][room["probes"]]
    lim = F(1) - H.T08
    up, dn = lambda x: np.nextafter(F(x), F(np.inf)), lambda x: np.nextafter(F(x), F(-np.inf))
    def at(y):
        return np.flatnonzero((nor[:, 1] == F(y)) & np.isfinite(nor[:, 0]) & np.isfinite(nor[:, 2]))
    assert len(at(H.T08)) and not fm[at(H.T08)].any() and fm[at(up(H.T08))].all() and not fm[at(dn(H.T08))].any()
    assert not wm[at(lim)].any() and not wm[at(up(lim))].any() and wm[at(dn(lim))].all() and wm[at(dn(-lim))].sum() == 0 and wm[at(up(-lim))].all()
    assert wm[at(0.0)].all() and len(at(0.0)) >= 4                                    # +0 and -0 compare equal: both are here
    bad = ~(np.isfinite(nor[:, 0]) & np.isfinite(nor[:, 2])) | np.isnan(nor[:, 1])
    assert bad.sum() >= 16 and not fm[bad].any() and not wm[bad].any()                 # the kept * 0.0f: NaN fails both compares
    # the band points are decided by the model they were made for, and some of them only by its arithmetic
    model = (golden["room_pos"][golden["room_r1_idx"][room["best"], 0]], room["model"][1])
    assert R.same_bits(model[0], room["model"][0])
    off = H.offset_variants(room["pos"][room["band"]], *room["model"])
    plain = H.inlier(off["plain"], room["dist_threshold"])
    removed = (golden["room_r1_mask_before"] == 1) & (golden["room_r1_mask_after"] == 0)
    assert (removed[room["band"]] == plain).all() and 40 <= plain.sum() <= H.N_BAND - 40
    assert (H.inlier(off["fma"], room["dist_threshold"]) != plain).sum() >= 1 and (H.inlier(off["pre"], room["dist_threshold"]) != plain).sum() >= 8
    # the tie cloud: maxima shared by hundreds of indices, in every round that detects something
    tie = H.tie_clouds(("t3",))[0]
    assert R.same_bits(tie["pos"], golden["tie_pos"]) and R.same_bits(tie["nor"], golden["tie_nor"])
    got = check_detection(golden, "tie_")
    for r in got["rounds"][:-1]:
        top = np.flatnonzero(r["counts"] == r["counts"].max())
        assert len(top) >= 256 and len(set(top % 256)) >= 128 and top[-1] - top[0] > 2000


def test_plain_offsets_are_the_restatement_bit_for_bit(cases):
    for name, c in cases.items():
        off = H.offset_variants(c["pos"], c["center"], c["normal"])["plain"]
        for h in range(len(c["center"])):
            want = R.offsets(c["pos"], c["center"][h], c["normal"][h]).astype(F)
            nan = np.isnan(want)
            assert (np.isnan(off[h]) == nan).all() and R.same_bits(off[h][~nan], want[~nan]), (name, h)
        one = H.offset_variants(c["pos"], c["center"][7], c["normal"][7])
        assert one["plain"].shape == (len(c["pos"]),) and one["plain"].tobytes() == off[7].tobytes()
        assert (H.variant_votes(c)["plain"] == R.votes(c["pos"], c["mask"], c["center"], c["normal"], c["dist_threshold"])).all(), name
    # the fused multiply-add is rounded once: 1 + 2^-24 + 2^-60 lies above the tie that a double rounding would round to even
    assert H.fma(F(1), F(1), F(2.0 ** -24)) == 1.0 and float(H.fma(F(1 + 2.0 ** -23), F(1 + 2.0 ** -23), F(-1))) == float(F(2.0 ** -22 + 2.0 ** -46))
    a = F(1 + 2.0 ** -12); assert float(H.fma(a, a, F(2.0 ** -60))) == 1 + 2.0 ** -11 + 2.0 ** -23    # a * a = 1 + 2^-11 + 2^-24 exactly


def test_gather_variants_plain_is_the_restatement():
    for name, family in H.GATHER_FAMILIES.items():
        c = family(257); M = c["models"]
        for m in range(len(M["center"])):
            with np.errstate(all="ignore"):
                want = ((c["nor"][:, 0] * M["normal"][m][0] + c["nor"][:, 1] * M["normal"][m][1]) + c["nor"][:, 2] * M["normal"][m][2]).astype(F)
            got = H.dot_variants(c["nor"], M["normal"][m])["plain"]
            assert R.same_bits(got, want), (name, m)
            poly = R.quad(M["center"][m], M["axes"][m], M["extends"][m])
            v = H.val_variants(c["pos"], poly)
            assert (~(v["plain"] < 0).any(axis=0) == R.within(c["pos"], poly)).all(), (name, m)


@pytest.mark.parametrize("name", ("band_0.01", "band_0.033", "band_3m_0.01", "band_3m_0.033"))
def test_band_families_hold_witnesses_for_every_variant(witnesses, name):
    w = witnesses[name]
    print(name, w)
    assert w["fma"] >= 8 and w["pre"] >= 8 and w["other"] >= 8, w


def test_far_family_holds_witnesses_for_the_precomputed_dot(witnesses, cases):
    print(witnesses["far"])
    assert witnesses["far"]["pre"] >= 8
    c = cases["far"]
    assert (c["center"][:3] < 0).all(axis=1).tolist() == [False, False, True] and np.abs(c["center"]).max() > 9e3


def test_witnesses_move_the_counts(cases):
    """What the GPU test asserts against: on every band family each variant's counts differ from the restatement's."""
    for name in ("band_0.01", "band_0.033", "band_3m_0.01", "band_3m_0.033", "far"):
        c = cases[name]
        for mname, m in H.vote_masks(c).items():
            v = H.variant_votes(c, m)
            assert (v["pre"] != v["plain"]).any(), (name, mname)
            if name != "far":
                assert (v["fma"] != v["plain"]).any() and (v["other"] != v["plain"]).any(), (name, mname)


def test_exact_family_counts_in_closed_form(cases):
    c = cases["exact"]
    want = c["inlier"].sum(axis=1)
    assert (R.votes(c["pos"], c["mask"], c["center"], c["normal"], c["dist_threshold"]) == want).all()
    d = c["design"]
    thr = c["dist_threshold"]
    # a point made for an axis and a centre component of 0 sits at +-thr, the float below or the float above: of a hypothesis along
    # that axis whose centre component is 0, only the float below is an inlier
    for h in range(len(c["center"])):
        k = d["h_axis"][h]
        if c["center"][h, k] != 0:
            continue
        own = (d["axis"] == k) & (d["cc"] == 0)
        assert c["inlier"][h][own & (d["kind"] == 1)].all() and not c["inlier"][h][own & (d["kind"] != 1)].any(), h
    assert np.abs(c["pos"][(d["axis"] == 0) & (d["cc"] == 0) & (d["kind"] == 0), 0]).tolist().count(float(thr)) > 0
    assert np.signbit(c["pos"][c["pos"] == 0]).any() and np.signbit(c["center"][c["center"] == 0]).any() and c["special"].any()
    assert want.min() > 0 and len(set(want.tolist())) > 3
    for mname, m in H.vote_masks(c).items():
        assert (R.votes(c["pos"], m, c["center"], c["normal"], thr) == (c["inlier"] & m.astype(bool)[None]).sum(axis=1)).all(), mname


def test_special_family_decides_as_ieee_does(cases):
    c = cases["special"]
    counts = R.votes(c["pos"], c["mask"], c["center"], c["normal"], c["dist_threshold"])
    finite = np.isfinite(c["pos"]).all(axis=1)
    assert c["special"].sum() == 64 and 20 <= (~finite).sum() < 64
    for what, j in c["swaps"].items():
        assert counts[j] == (finite.sum() if "zero_normal" in what else 0), what
    for mname, m in H.vote_masks(c).items():
        assert R.votes(c["pos"], m, c["center"], c["normal"], c["dist_threshold"])[1] == (finite & m.astype(bool)).sum(), mname
    ordinary = np.setdiff1d(np.arange(len(counts)), list(c["swaps"].values()))
    assert counts[ordinary].max() > 100


def test_subnormal_block_shows_a_flush_to_zero(cases):
    c = cases["special_subnormal"]
    counts = R.votes(c["pos"], c["mask"], c["center"], c["normal"], c["dist_threshold"])
    assert 0 < float(c["dist_threshold"]) < H.FLT_MIN and np.abs(c["normal"]).max() < 1e-19
    with np.errstate(all="ignore"):
        prod = np.abs(c["normal"][:, None, :] * (c["pos"][None, :, :] - c["center"][:, None, :]))
    assert prod.max() < H.FLT_MIN and (prod > 0).mean() > 0.99
    flushed = H.flushed_votes(c)
    assert (counts != flushed).all() and counts.min() > 100 and counts.max() < len(c["pos"]) - 100 and (flushed == 0).all()


def test_dot_band_holds_witnesses_for_the_normal_dot():
    c = H.dot_band(2049)
    w8, w0 = H.gather_witnesses(c, 0.8), H.gather_witnesses(c, 0.0)
    print(w8, w0)
    assert w8["fma"] >= 8 and w8["other"] >= 8
    assert w0["fma"] >= 8 and w0["other"] >= 8                   # the relabel's > 0.0f: the near-perpendicular normals
    M = c["models"]
    own3 = np.arange(2049) % 4 == 3
    with np.errstate(all="ignore"):
        dot = ((c["nor"][:, 0] * M["normal"][3][0] + c["nor"][:, 1] * M["normal"][3][1]) + c["nor"][:, 2] * M["normal"][3][2])[own3]
    assert (dot == 0).sum() >= 100 and np.signbit(dot[dot == 0]).any() and not np.signbit(dot[dot == 0]).all()
    assert ((np.abs(dot) > 0) & (np.abs(dot) < H.FLT_MIN)).sum() >= 50                 # subnormal products: inliers unless flushed


def test_quad_edges_hold_witnesses_and_show_the_untested_edge():
    c = H.quad_edges(2049)
    w = H.quad_witnesses(c)
    print(w)
    assert w >= 4
    M = c["models"]
    for m in (0, 1, 3, 4):
        own = c["owner"] == m
        kept = R.inlier_flags(c["pos"], c["nor"], M["center"][m], M["normal"][m], M["axes"][m], M["extends"][m], 0.8, 0.05, True)
        beyond = [kept[own & (c["place"] == 8 + j)] for j in range(4)]
        assert all(len(b) >= 30 for b in beyond)
        assert not beyond[0].any() and not beyond[1].any() and not beyond[2].any() and beyond[3].all(), m      # 0.3 m beyond the fourth edge: kept
        on_edges = kept[own & (c["place"] < 8)]
        assert on_edges.any() and not on_edges.all(), m
    own = c["owner"] == 2                                                                                     # the degenerate quad keeps everybody
    assert R.within(c["pos"][own], R.quad(M["center"][2], M["axes"][2], M["extends"][2])).all()
    assert (M["extends"][3] * M["extends"][1] < 0).all() and np.signbit(M["axes"][4][M["axes"][4] == 0]).any()


def test_labels_family_shows_the_order_of_application():
    c = H.labels(2049); M = c["models"]
    args = (c["pos"], c["nor"], M["center"], M["normal"], M["axes"], M["extends"])
    cls, inst = R.relabel(*args, M["valid"], M["up_dot"], *c["ids"], c["cls"], c["inst"])
    assert M["valid"].tolist() == [1, 0, 1, 1] and M["up_dot"][0] == H.T08 and M["up_dot"][2] > H.T08 and np.isnan(M["up_dot"][3])
    for v in (1023, 1024, H.INT32_MAX, H.INT32_MIN, -1):
        assert (c["inst"] == v).any()
    assert (inst[c["inst"] < 1024] == c["inst"][c["inst"] < 1024]).all() and (cls[c["cls"] != 0] == c["cls"][c["cls"] != 0]).all()
    assert (inst == 0).any() and (inst[c["inst"] >= 1024] == 1).any() and (cls[c["cls"] == 0] == 2).any() and (cls[c["cls"] == 0] == 1).any()
    # other orders and the invalid model applied give other ids
    rev = [2, 1, 0, 3]
    other = R.relabel(c["pos"], c["nor"], *[M[k][rev] for k in ("center", "normal", "axes", "extends", "valid", "up_dot")], *c["ids"], c["cls"], c["inst"])
    assert (other[0] != cls).any() and (other[1] != inst).any()
    allv = R.relabel(*args, np.ones(4, np.int8), M["up_dot"], *c["ids"], c["cls"], c["inst"])
    assert (allv[0] != cls).any() or (allv[1] != inst).any()
    floor_at_08 = M["up_dot"].copy(); floor_at_08[0] = np.nextafter(H.T08, F(1))
    assert (R.relabel(*args, M["valid"], floor_at_08, *c["ids"], c["cls"], c["inst"])[0] != cls).any()


def test_tie_clouds_have_their_index_properties():
    clouds = {c["name"]: c for c in H.tie_clouds()}
    assert [int((R.candidate_masks(clouds[k]["nor"], H.T08)[0]).sum()) for k in ("t3", "t4", "t5_late", "t5_last")] == [3, 4, 5, 5]
    for name, c in clouds.items():
        got = R.detect(c["pos"], c["nor"], 0.8, 0.033, c["count_threshold"])
        r0, r1 = got["rounds"][0], got["rounds"][1]
        top0 = np.flatnonzero(r0["counts"] == r0["counts"].max())
        assert len(r0["idx"]) == 2500 and len(r1["idx"]) == 5000 and len(got["rounds"]) >= 3
        assert len(top0) >= 256 and len(set(top0 % 256)) >= 128, name                 # the floor: duplicates in every lane and stride
        top1 = np.flatnonzero(r1["counts"] == r1["counts"].max())
        if name in ("t3", "t4"):
            assert len(top1) >= 256 and len(set(top1 % 256)) >= 128 and r1["best"] == top1[0], name
        if name == "t5_late":
            assert r1["best"] == top1[0] >= 256 and r1["counts"][:top1[0]].max() < r1["counts"].max()
        if name == "t5_last":
            assert top1.tolist() == [4999] and r1["best"] == 4999
