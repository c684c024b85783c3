"""Host rehearsal of the signed running minimum (robosuite_amd/csrc/rsim_pen_clear_core.h clear_pairs_signed, the code k_clear_dist_signed runs per candidate) under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/signed_clear_core_driver.cpp is built with g++ and run as a subprocess.  Nothing sanitized is loaded
into Python.

Candidates, as lists of pair records rounded to fp32: the 210 of penetration_scenes.arm_cases(3, 70), half of them sunk 2 to 5 mm into the last link's capsule
(the exact branch), and the 80 sunk starts of tests/signed_query_scenes.py -- into a box (the descent runs) or a capsule; where TWO of a start's pairs are below
zero its list is ordered so that the SHALLOWER overlap comes first.  Those doubles are all capsule pairs, whose depth is exact from the cores' distance; so CONSTRUCTED lists, in which the deeper pair descends,
follow: the overlapping record of a start sunk into the box b3 behind the overlapping record of another start (into c2 or b3) that is at least 0.5 mm
shallower, and behind them three records of the first start that are free.  Every list is run a second time in reversed order.

Pass = the sanitizers report nothing and every call returns, and
  * clear_pairs_signed returns, bit for bit, the smallest pair_signed value over the same records with every pair queried at the call's distmax, and the lowest
    index that attains it: the running minimum loses nothing;
  * THE ORDER TEST: the reversed list gives the same dist bit for bit, and the same pair mapped back (where the mirror's two smallest values are not tied): the
    pair routine is never handed a negative distmax, so what a pair returns does not depend on what came before it.  (Tried on these lists: the running
    minimum handed on as it is passes too.  GJK's lower bound stays valid below zero, so the far exit drops a pair only where its TRUE depth is smaller than
    the minimum so far while the descent's local minimum is larger; no list here holds such a pair.  The first item is what holds the definition.);
  * against the fp64 mirror on the same records: a candidate the mirror sees free of overlaps within TOL + 2e-5 m (tests/test_distance_core_host.py's bound for
    the GJK core), one with an overlap within 4.7e-4 m, four times the 1.176e-4 m one device run of this very pair routine measured against this very mirror
    (tests/test_penetration.py BOUND["dist"], profiles/penetration_parity.txt); the pair equal unless the mirror's two smallest values lie within that bound;
  * no status carries OVERLAP, a sunk candidate has dist < 0."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from robosuite_amd import distance as D
from robosuite_amd import clearance
from robosuite_amd import penetration as P
from tests import distance_scenes as S
from tests import penetration_scenes as Q
from tests import signed_query_scenes as SQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "signed_clear_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TOL, MAX_ITERS, DISTMAX = D.DEFAULTS["tol"], D.DEFAULTS["max_iters"], 1.0
FREE_BOUND, PEN_BOUND = TOL + 2e-5, 4 * 1.176e-4
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
B, K = 3, 70


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("signed_clear_san") / "signed_clear_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def records(flat, qpos, dofs, q, pairs, params):
    xpos, xquat = clearance.fk(flat, qpos, dofs, q)
    G = D.world_geoms(flat, xpos, xquat, np.asarray(pairs).ravel(), params)
    return [(S.geom32(G[int(a)]), S.geom32(G[int(b)])) for a, b in pairs]


def run(exe, tmp, cands, **pen):
    o = P.options(pen)
    fin, fout = os.path.join(str(tmp), "cands.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<iffifif", len(cands), DISTMAX, TOL, MAX_ITERS, o["pen_tol"], o["pen_iters"], o["offset"]))
        for recs in cands:
            f.write(struct.pack("<i", len(recs)) + S.pack_records(recs, DISTMAX, TOL, MAX_ITERS)[16:])
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash, every candidate returned
    print("driver:", r.stdout.strip())
    with open(fout, "rb") as f:
        rec = np.frombuffer(f.read(), dtype=np.dtype([("f", "<f4", 8), ("i", "<i4", 4)]), count=len(cands))
    return dict(dist=rec["f"][:, 0], fromto=rec["f"][:, 1:7], brute=rec["f"][:, 7], pair=rec["i"][:, 0], status=rec["i"][:, 1], steps=rec["i"][:, 2], brute_pair=rec["i"][:, 3])


def mirror(recs):
    """the per-pair signed values of one candidate on the fp64 mirror, far pairs at +inf"""
    o = P.options(None)
    out = np.full(len(recs), np.inf)
    for i, (a, b) in enumerate(recs):
        d, _, st = P.pair_signed(a, b, DISTMAX, TOL, MAX_ITERS, **o)
        out[i] = np.inf if st & D.FAR else d
    return out


@pytest.fixture(scope="module")
def data(exe, tmp_path_factory):
    c = Q.arm_cases(B, K)
    params = S.params32(c["flat"])
    lists, sunk = [], []
    for e in range(B):
        for k in range(K):
            lists.append(records(c["flat"], c["qpos"][e], c["dofs"], c["q"][e, k], c["pairs"], params))
            sunk.append(bool(c["sunk"][e, k]))
    s = SQ.cases()
    two = []
    for e, k in np.argwhere(s["nneg"] >= 1):
        recs = records(s["flat"], s["qpos"][e], s["dofs"], s["q_init"][e, k], s["pairs"], params)
        if s["nneg"][e, k] > 1:
            a, b = np.argsort(mirror(recs))[:2]      # deepest, second deepest: both below zero
            if a < b:      # the shallower of the two comes first
                recs[a], recs[b] = recs[b], recs[a]
            two.append(len(lists))
        lists.append(recs)
        sunk.append(True)
    # constructed: [a shallower overlap, a deeper box x box overlap, three free records]
    starts = [(lists[i], mirror(lists[i])) for i in range(B * K, len(lists))]
    deep = [(recs, m) for (recs, m), (e, k) in zip(starts, np.argwhere(s["nneg"] >= 1)) if e % 2 == 0 and s["nneg"][e, k] == 1]      # sunk into b3 alone
    built = []
    for i, (rb, mb) in enumerate(deep):
        for rs, ms in starts[i % 7::7]:
            if (ms < 0).sum() == 1 and ms.min() - mb.min() >= 5e-4:
                free = [rb[j] for j in np.flatnonzero(mb > 0)[:3]]
                built.append(len(lists))
                lists.append([rs[int(np.argmin(ms))], rb[int(np.argmin(mb))]] + free)
                sunk.append(True)
    ref = [mirror(recs) for recs in lists]
    fwd = run(exe, tmp_path_factory.mktemp("signed_clear_fwd"), lists)
    rev = run(exe, tmp_path_factory.mktemp("signed_clear_rev"), [recs[::-1] for recs in lists])
    return dict(lists=lists, sunk=np.array(sunk), ref=ref, fwd=fwd, rev=rev, two=two, built=built)


def test_running_minimum_is_the_plain_minimum_of_pair_signed(data):
    for r in (data["fwd"], data["rev"]):
        assert np.array_equal(r["dist"], r["brute"]) and np.array_equal(r["pair"], r["brute_pair"])
        assert not (r["status"] & D.OVERLAP).any() and not (r["status"] & (D.CAP | P.PEN_CAP)).any()
        assert (r["dist"][data["sunk"]] < 0).all() and (r["pair"] >= 0).all()


def test_order_of_the_list_does_not_change_the_result(data):
    fwd, rev, two = data["fwd"], data["rev"], data["two"]
    assert len(two) >= 5      # candidates with two overlapping pairs, the shallower first
    assert np.array_equal(fwd["dist"], rev["dist"])
    tied = 0
    for i, m in enumerate(data["ref"]):
        s = np.sort(m)
        if s[1] - s[0] <= PEN_BOUND:
            tied += 1
            continue
        assert rev["pair"][i] == len(m) - 1 - fwd["pair"][i], i
    first = [bool(np.sort(data["ref"][i])[1] < 0 and np.argsort(data["ref"][i])[1] < np.argsort(data["ref"][i])[0]) for i in two]
    print(f"{len(data['lists'])} candidates in both orders, {len(two)} with two pairs below zero ({sum(first)} of them with the shallower first), {tied} with the two "
          f"smallest within the bound; {(fwd['steps'] > 0).sum()} candidates descended, {(fwd['steps'][two] > 0).sum()} of them with two pairs below zero")
    assert all(first)
    built = data["built"]      # the shallower overlap first, the deeper box pair -- whose cores overlap: the descent -- second
    assert len(built) >= 10 and (fwd["pair"][built] == 1).all() and (rev["pair"][built] == len(data["lists"][built[0]]) - 2).all() and (fwd["steps"][built] > 0).all()
    assert all(data["ref"][i][0] < 0 and data["ref"][i][1] < data["ref"][i][0] for i in built)
    assert (fwd["steps"] > 0).sum() >= 20


def test_against_the_mirror(data):
    fwd, sunk = data["fwd"], data["sunk"]
    md = np.array([m.min() for m in data["ref"]])
    mp = np.array([int(np.argmin(m)) for m in data["ref"]])
    gap = np.array([np.sort(m)[1] - np.sort(m)[0] for m in data["ref"]])
    err = np.abs(fwd["dist"].astype(np.float64) - md)
    over = md < 0
    print(f"fp32 running minimum on the host: {len(md)} candidates, {over.sum()} below zero; |dist - mirror| worst {err[over].max():.3e} (bound {PEN_BOUND:.1e}) where "
          f"a pair overlaps, {err[~over].max():.3e} (bound {FREE_BOUND:.1e}) elsewhere")
    assert over[sunk].all()      # (a uniform candidate may stand below zero too: through the floor, capsule in capsule -- exact without descent)
    assert err[over].max() <= PEN_BOUND and err[~over].max() <= FREE_BOUND
    assert (fwd["pair"] == mp)[gap > PEN_BOUND].all()
    for i in np.flatnonzero(sunk)[::5]:      # the witnesses of a sunk candidate carry the direction the gradient reads: unit, and along it the records come free
        a, b = data["lists"][i][fwd["pair"][i]]
        ft, d = fwd["fromto"][i].astype(np.float64), float(fwd["dist"][i])
        n = (ft[3:] - ft[:3]) / d
        assert abs(np.linalg.norm(n) - 1) <= 2e-4, i      # six fp32 coordinates up to 1 m, 2^-24 each, over a depth of 2e-3 m
        assert Q.separates(a, b, d, n / np.linalg.norm(n), slack=2e-6 + TOL), i
