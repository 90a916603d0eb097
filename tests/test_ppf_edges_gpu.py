"""The PPF kernels (csrc/ppf.hip) at their edges: every case of tests/ppf_cases.py through ossid_ppf_sample, _model_table,
_scene_normals, _vote and _cluster directly, against the restatement tests/ref_ppf.py, with SPEC 6.8's assertions:
bit-equal indices, points, normals, counts, stats, table multisets, peaks, poses, scores and info; scene normals within
1e-6 rad of eigh where the eigenvalue gap allows it; zero rows past the live ones; guard words behind every output
untouched; two runs byte-identical."""
import numpy as np
import pytest
import torch

import ppf_cases as pc
import ref_ppf as rp

pytestmark = pytest.mark.gpu

G = 8                                                   # guard rows behind every output
GI, GF = -7, 777.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guard(rows, tail, dtype):
    """an output of `rows` rows (+ G guard rows), filled with the guard value"""
    v = GF if dtype in (torch.float32, torch.float64) else GI
    return torch.full((rows + G,) + tuple(tail), v, dtype=dtype, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def untouched(a, start):
    a = a[start:]
    return bool(np.all(a == (GF if a.dtype.kind == "f" else GI)))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- sampling -----------------------------------------------------------------------------------------------------------
def run_sample(lib, c):
    n_in, mo = c["n_in"], c["max_out"]
    wsb = lib.fn("ossid_ppf_sample_workspace_bytes")(n_in)
    assert wsb > 0
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    model = c.get("normals") is not None
    o = dict(idx=guard(mo, (), torch.int32), pts=guard(mo, (3,), torch.float32), count=guard(1, (), torch.int32),
             stats=guard(8, (), torch.float32), nrm=guard(mo, (3,), torch.float32) if model else None)
    if c["form"] == "depth":
        H, W = c["depth"].shape
        K = c["K"]
        ins = [dev(c["depth"]), dev(c["mask"])]
        args = (None, None, 0, ins[0].data_ptr(), ins[1].data_ptr(), H, W, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    else:
        ins = [dev(c["points"].astype(np.float32)), dev(c["normals"].astype(np.float32)) if model else None]
        args = (ins[0].data_ptr(), ins[1].data_ptr() if model else None, n_in, None, None, 0, 0, 1.0, 1.0, 0.0, 0.0)
    rc = lib.fn("ossid_ppf_sample")(*args, c["rel"], c["diam"], mo, ws.data_ptr(), wsb, o["idx"].data_ptr(), o["pts"].data_ptr(),
                                    o["nrm"].data_ptr() if model else None, o["count"].data_ptr(), o["stats"].data_ptr(), None)
    assert rc == 0
    out = {k: host(v) for k, v in o.items() if v is not None}
    assert np.all(host(ws)[wsb:] == 0x5A)
    return out


def check_sample(out, want, mo, src=None):
    k = min(want["count"], mo)
    assert out["count"][0] == want["count"] and untouched(out["count"], 1)
    idx = out["idx"][:k] if src is None else src[out["idx"][:k]]
    assert same(idx, want["idx"][:k]) and untouched(out["idx"], k)
    assert same(out["pts"][:k], want["pts"][:k]) and untouched(out["pts"], k)
    if want["nrm"] is not None:
        assert same(out["nrm"][:k], want["nrm"][:k]) and untouched(out["nrm"], k)
    assert same(out["stats"][:8], want["stats"]) and untouched(out["stats"], 8)


@pytest.mark.parametrize("name", pc.NAMES["sample"])
def test_sample(hiplib, name):
    c = pc.by_name("sample")[name]
    a, b = run_sample(hiplib, c), run_sample(hiplib, c)
    check_sample(a, c["want"], c["max_out"])
    assert all(same(a[k], b[k]) for k in a)
    if c["form"] == "depth":                            # the cloud form of the same pixels keeps the same points
        twin, pix = pc.cloud_twin(c)
        t = run_sample(hiplib, twin)
        check_sample(t, dict(c["want"], idx=c["want"]["idx"]), c["max_out"], src=pix.astype(np.int32))
        assert same(t["pts"], a["pts"]) and same(t["stats"], a["stats"])


# ---- model table --------------------------------------------------------------------------------------------------------
def run_table(lib, c):
    Ms, words = c["Ms"], c["words"]
    assert lib.fn("ossid_ppf_model_table_words")(Ms, float(c["h"]), float(c["D"])) == words
    P, N = dev(c["P"]), dev(c["N"])
    ne = max(Ms * (Ms - 1), 1)
    off, ent, ws = guard(words, (), torch.int32), guard(ne, (), torch.int32), guard(words, (), torch.int32)
    rc = lib.fn("ossid_ppf_model_table")(P.data_ptr(), N.data_ptr(), Ms, float(c["h"]), float(c["D"]), off.data_ptr(), ent.data_ptr(),
                                         ne, ws.data_ptr(), words * 4, None)
    assert rc == 0
    assert untouched(host(ws), words)
    return host(off), host(ent)


@pytest.mark.parametrize("name", pc.NAMES["table"])
def test_model_table(hiplib, name):
    c = pc.by_name("table")[name]
    m, nch, words = c["model"], c["nch"], c["words"]
    off, ent = run_table(hiplib, c)
    assert untouched(off, words) and off[0] == 0 and off[words - 1] == len(m.entries) and np.all(np.diff(off[:words]) >= 0)
    assert untouched(ent, len(m.entries))               # entries past the last range are never written
    o = off[:words].astype(np.int64)
    e = ent[:len(m.entries)].view(np.uint32)
    slot = np.repeat(np.arange(words - 1), np.diff(o))
    assert np.array_equal(slot % nch, (e >> 5) // pc.CHUNK)               # each entry in its reference point's chunk
    o_dev, o_ref = np.lexsort((e, slot // nch)), np.lexsort((m.entries, m.keys))
    assert np.array_equal((slot // nch)[o_dev], m.keys[o_ref]) and np.array_equal(e[o_dev], m.entries[o_ref])
    off2, ent2 = run_table(hiplib, c)                   # the offsets are reproducible; the order within a range is unspecified
    assert same(off, off2) and np.array_equal(np.sort(ent2[:len(m.entries)]), np.sort(ent[:len(m.entries)]))


def test_model_table_refuses_129_distance_bins(hiplib):
    c = pc.TABLE_EINVAL
    assert hiplib.fn("ossid_ppf_model_table_words")(c["Ms"], float(c["h"]), float(c["D"])) == 0
    P = dev(pc.lattice(2, 2, 2, 8.0))
    out = guard(1 << 16, (), torch.int32)
    p = out.data_ptr()
    rc = hiplib.fn("ossid_ppf_model_table")(P.data_ptr(), P.data_ptr(), c["Ms"], float(c["h"]), float(c["D"]), p, p, 1 << 16, p, 1 << 18, None)
    assert rc == pc.EINVAL and untouched(host(out), 0)  # refused before any launch: nothing is written
    assert hiplib.fn("ossid_ppf_model_table_words")(c["Ms"], float(c["h"]), float(pc.down(c["D"]))) == 128 * 3375 + 1


# ---- scene normals ------------------------------------------------------------------------------------------------------
def run_normals(lib, c):
    S, cnt = dev(c["S"]), dev(np.array([c["count"]], dtype=np.int32))
    nrm, ok = guard(c["cap"], (3,), torch.float32), torch.full((c["cap"] + G,), 0x5A, dtype=torch.uint8, device="cuda")
    assert lib.fn("ossid_ppf_scene_normals")(S.data_ptr(), cnt.data_ptr(), c["cap"], float(c["radius"]), nrm.data_ptr(), ok.data_ptr(), None) == 0
    return host(nrm), host(ok)


def angle(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), rp._dot(a, b))


@pytest.mark.parametrize("name", pc.NAMES["normals"])
def test_scene_normals(hiplib, name):
    c = pc.by_name("normals")[name]
    n, cap, w = c["n"], c["cap"], c["want"]
    nrm, ok = run_normals(hiplib, c)
    nrm2, ok2 = run_normals(hiplib, c)
    assert same(nrm, nrm2) and same(ok, ok2)
    assert untouched(nrm, cap) and np.all(ok[cap:] == 0x5A)
    assert np.array_equal(ok[:n], w["ok"].astype(np.uint8)) and not ok[n:cap].any()
    assert not nrm[:cap][ok[:cap] == 0].any()          # dropped points and rows past count: zero normals
    good = np.flatnonzero(w["ok"])
    if len(good) == 0:
        return
    a, S = nrm[good], c["S"][good]
    assert np.all(np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0) <= 1e-6)
    assert np.all(rp._dot(a, S) <= 0)                   # the sign rule, in f32
    if "pinned" in c:
        assert same(a, c["pinned"][good])
    if c["loose"]:                                      # marked by the builder: the direction is not unique, or only up to sign
        if "pinned" in c:
            assert np.all(angle(a, np.abs(w["nrm"][good])) <= 1e-6)
        return
    worst = float(angle(a, w["nrm"][good]).max())
    print("%s: largest normal gap %.3e rad over %d normals (eigenvalue gap >= %.3f)" % (name, worst, len(good), c["premise"]["min_gap"]))
    assert worst <= 1e-6


# ---- vote ---------------------------------------------------------------------------------------------------------------
def run_vote(lib, c, table):
    m = c["model"]
    off, ent = table
    P, N, S, Sn, Sok = dev(m.P), dev(m.N), dev(c["S"]), dev(c["Sn"]), dev(c["Sok"])
    cnt = dev(np.array([c["n"]], dtype=np.int32))
    wsb = lib.fn("ossid_ppf_vote_workspace_bytes")(c["cap"], c["ref_step"], c["Ms"])
    assert wsb == c["max_ref"] * c["nch"] * 8
    ws = guard(wsb // 4, (), torch.int32)
    peaks, poses = guard(c["max_ref"], (3,), torch.int32), guard(c["max_ref"], (4, 4), torch.float64)
    rc = lib.fn("ossid_ppf_vote")(S.data_ptr(), Sn.data_ptr(), Sok.data_ptr(), cnt.data_ptr(), c["cap"], c["ref_step"], P.data_ptr(),
                                  N.data_ptr(), c["Ms"], float(m.h), float(m.D), off.data_ptr(), ent.data_ptr(), ws.data_ptr(), wsb,
                                  peaks.data_ptr(), poses.data_ptr(), None)
    assert rc == 0
    assert untouched(host(ws), wsb // 4)
    return host(peaks), host(poses)


@pytest.mark.parametrize("name", pc.NAMES["vote"])
def test_vote(hiplib, name):
    c = pc.by_name("vote")[name]
    off, ent = pc.host_table(c["model"], c["nch"])
    table = (dev(off.view(np.int32)), dev(np.concatenate([ent, np.zeros(1, np.uint32)]).view(np.int32)))
    peaks, poses = run_vote(hiplib, c, table)
    k, w = c["max_ref"], c["want"]
    assert untouched(peaks, k) and untouched(poses, k)
    bad = np.flatnonzero((peaks[:k] != w["peaks"]).any(1))
    assert len(bad) == 0, (bad[:5], peaks[bad[:5]], w["peaks"][bad[:5]])
    assert same(poses[:k], w["poses"])                  # identity where there is no candidate, slots past n included
    peaks2, poses2 = run_vote(hiplib, c, table)
    assert same(peaks, peaks2) and same(poses, poses2)


# ---- cluster ------------------------------------------------------------------------------------------------------------
def run_cluster(lib, c):
    pk, cp, cnt = dev(c["peaks"]), dev(c["cand_poses"]), dev(np.array([c["count"]], dtype=np.int32))
    nr = c["num_result"]
    poses, scores, info = guard(nr, (4, 4), torch.float64), guard(nr, (), torch.float64), guard(4, (), torch.int32)
    rc = lib.fn("ossid_ppf_cluster")(pk.data_ptr(), cp.data_ptr(), cnt.data_ptr(), c["cap"], c["ref_step"], c["Ms"], float(c["D"]),
                                     float(c["dist_rel"]), nr, poses.data_ptr(), scores.data_ptr(), info.data_ptr(), None)
    assert rc == 0
    return host(poses), host(scores), host(info)


@pytest.mark.parametrize("name", pc.NAMES["cluster"])
def test_cluster(hiplib, name):
    c = pc.by_name("cluster")[name]
    w, nr = c["want"], c["num_result"]
    poses, scores, info = run_cluster(hiplib, c)
    assert same(info[:4], w["info"]) and untouched(info, 4) and untouched(poses, nr) and untouched(scores, nr)
    k = int(info[0])
    assert k == len(w["poses"]) == min(c["premise"]["nseed"], nr)
    assert same(scores[:k], w["scores"]), np.flatnonzero(scores[:k] != w["scores"])[:5]
    assert same(poses[:k], w["poses"])
    assert not poses[k:nr].any() and not scores[k:nr].any()               # result rows past info[0] are zero
    again = run_cluster(hiplib, c)
    assert same(poses, again[0]) and same(scores, again[1]) and same(info, again[2])
