"""csrc/sc_plan.h -- the integer logic that cuts a query batch into host-entry pieces, filter batches and the XCD-aware work
split of the two-wave filter kernel -- compiled with the host compiler and checked over a sweep of sizes: every query / every
(tile-block, query tile) unit is covered exactly once, the shapes are the documented ones.  Likewise the decisions the query
entries of csrc/sc_api.cpp take from it: which kernels score a batch (at every threshold edge), a shard's share of the indices,
the stage-1 share and the padded leading dimension."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "sc_plan.h"
using namespace rsx::sc::plan;
int main() {
  std::printf("{\"pieces\": [");
  const int nqs[] = {1, 63, 64, 1000, 4095, 4096, 4097, 5555, 8192, 10000, 65536, 1000000};
  bool first = true;
  for (int nq : nqs) for (int f : {0, 256, 1024}) for (int g : {5, 10, 25, 40}) {
    int32_t sz[8];
    const int n = host_pieces(nq, f, g, 8, sz);
    std::printf("%s[%d, %d, %d, [", first ? "" : ", ", nq, f, g);
    first = false;
    for (int i = 0; i < n; i++) std::printf("%s%d", i ? ", " : "", sz[i]);
    std::printf("]]");
  }
  std::printf("], \"batches\": [");
  first = true;
  for (long long n : {1ll, 970ll, 9970ll, 99970ll, 1000000ll, 40000000ll}) for (long long nq : {1ll, 64ll, 100ll, 8192ll, 100000ll}) {
    std::printf("%s[%lld, %lld, %lld]", first ? "" : ", ", n, nq, (long long)filter_batch(n, nq));
    first = false;
  }
  std::printf("], \"xcd\": [");
  first = true;
  for (long long nq : {64ll, 511ll, 512ll, 1024ll, 3200ll, 4608ll, 8192ll, 8189ll, 100000ll}) for (long long n : {1250ll, 9970ll, 99970ll}) for (int cu : {256, 304, 250}) {
    const long long nqt = (nq + 3) / 4, ntb = ((n + 31) / 32 + 3) / 4;
    const XcdSplit s = xcd_split(nqt, ntb, cu);
    std::printf("%s[%lld, %lld, %d, %d, %d, %d, %u]", first ? "" : ", ", nqt, ntb, cu, s.on ? 1 : 0, s.nqt_x, s.len, s.grid);
    first = false;
  }
  std::printf("], \"owned\": [");
  first = true;
  for (int w = 1; w <= 9; w++) for (int r = 0; r < w; r++) for (int n = 0; n <= 40; n++) {
    std::printf("%s[%d, %d, %d, %lld]", first ? "" : ", ", w, r, n, (long long)owned_below(n, r, w));
    first = false;
  }
  std::printf("], \"paths\": [");
  first = true;
  for (int m = 0; m <= 3; m++) for (int nq : {1, 2, 8, 9, 16, 17, 64})
    for (long long e : {0ll, (1ll << 17) / nq, 400000ll / nq, 800000ll / nq, 50000ll}) for (long long n = e > 0 ? e - 1 : 0; n <= e + 1; n++) {
      const int with = (int)query_path(m, nq, n), without = (int)query_path(m, nq, n, false);
      const Stage1Plan s1 = stage1_plan(m, nq, n);
      std::printf("%s[%d, %d, %lld, %d, %d, %d, %d, %d]", first ? "" : ", ", m, nq, n, with, without, one_tail(query_path(m, nq, n), n, nq) ? 1 : 0,
                  s1.split ? 1 : 0, (int)s1.whole);
      first = false;
    }
  std::printf("], \"path_names\": [%d, %d, %d], \"share\": [", (int)Path::SingleQuery, (int)Path::FilterChain, (int)Path::ExactAll);
  for (int w = 1; w <= 64; w++) std::printf("%s[%d, %d]", w > 1 ? ", " : "", w, stage1_share(160, w));
  std::printf("], \"ld\": [");
  first = true;
  for (long long n : {0ll, 1ll, 31ll, 32ll, 33ll, 970ll, 9970ll, 99970ll, 1000000ll, 40000000ll}) {
    std::printf("%s[%lld, %lld]", first ? "" : ", ", n, (long long)padded_ld(n));
    first = false;
  }
  std::printf("]}\n");
  return 0;
}
'''


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "navtech-radar-slam_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)


def test_host_pieces_cover_the_batch(plans):
    for nq, first, growth, sizes in plans["pieces"]:
        assert sum(sizes) == nq and all(s > 0 for s in sizes) and len(sizes) <= 8, (nq, first, growth, sizes)
        if first <= 0 or nq < 4 * first:
            assert sizes == [nq]
        else:
            assert all(s % 64 == 0 for s in sizes[:-1]) and sizes[0] == (first + 63) // 64 * 64
            if growth >= 10 and len(sizes) < 8:
                assert all(b >= a for a, b in zip(sizes[:-2], sizes[1:-1]))      # pieces do not shrink (the last takes the rest)
    # the shipped plan on the bench batch
    assert [s for nq, f, g, s in plans["pieces"] if (nq, f, g) == (8192, 1024, 25)] == [[1024, 2560, 4608]]


def test_filter_batches_are_even_and_bounded(plans):
    for n, nq, qb in plans["batches"]:
        ld = (n + 31) // 32 * 32
        assert 1 <= qb <= nq or (nq < 64 and qb == nq)
        if qb < nq:
            assert qb % 64 == 0 and (qb * ld <= 2 ** 29 or qb == 64)             # <= 1 GiB of fp16 bounds (64 queries at least)
            nb = -(-nq // qb)
            assert nq - (nb - 1) * qb > qb // 2 or nb == 1 or nb >= 8, (n, nq, qb)   # no stub of a last batch among a few
    assert [qb for n, nq, qb in plans["batches"] if (n, nq) == (99970, 8192)] == [4096]


def test_xcd_split_covers_every_unit_once(plans):
    used_somewhere = False
    for nqt, ntb, cu, on, nqt_x, ln, grid in plans["xcd"]:
        if not on:
            continue
        used_somewhere = True
        if ntb * nqt > 2_000_000:
            continue                                                              # (the sweep below is pure Python)
        assert cu % 8 == 0 and nqt_x == -(-nqt // 8) and ln >= 1 and grid % 8 == 0
        seen = set()
        for b in range(grid):                                                     # the kernel's own arithmetic (sc_spec.hip)
            x, j = b & 7, b >> 3
            sub, utb = divmod(j, ntb)
            qx1 = min((x + 1) * nqt_x, nqt)
            u0 = x * nqt_x + sub * ln
            u1 = min(u0 + ln, qx1)
            for u in range(u0, max(u0, u1)):
                assert (utb, u) not in seen
                seen.add((utb, u))
        assert len(seen) == ntb * nqt, (nqt, ntb, cu)
    assert used_somewhere
    # the bench launch: 2048 query tiles x 78 tile-blocks on 256 CUs -> two sub-ranges of 128 tiles per XCD
    assert [r[3:] for r in plans["xcd"] if r[:3] == [2048, 78, 256]][0] == [1, 256, 128, 8 * 2 * 78]
    # a 1024-query piece keeps the contiguous split (whole rounds would cost 17 %)
    assert [r[3] for r in plans["xcd"] if r[:3] == [256, 78, 256]] == [0]


def test_owned_below_counts_a_shards_indices(plans):
    """owned_below(n, rank, world) = |{i < n : i % world == rank}|: what the eligibility count, the appended range and the file
    check of a shard each used to work out for themselves"""
    table = {}
    for world, rank, n, got in plans["owned"]:
        assert got == sum(1 for i in range(n) if i % world == rank), (world, rank, n)
        table[world, rank, n] = got
    assert len(table) == sum(range(1, 10)) * 41
    # appending n keyframes at g0: the shard takes the owned indices of [g0, g0 + n)
    for world in range(1, 10):
        for rank in range(world):
            for g0 in range(0, 21):
                for n in range(0, 21):
                    want = sum(1 for i in range(g0, g0 + n) if i % world == rank)
                    assert table[world, rank, g0 + n] - table[world, rank, g0] == want, (world, rank, g0, n)


def _path_before(mode, nq, n, single_query=True):
    """the choice as the entries made it before it moved to sc_plan.h: use_q1, then use_filter, else exact-all"""
    q1 = single_query and 1 <= nq <= 16 and mode in (0, 3) and (mode == 3 or nq == 1 or nq * n <= (800000 if nq <= 8 else 400000))
    if q1:
        return "single"
    chain = not (mode == 1 or n <= 0) and (mode == 2 or n >= 50000 or nq * n >= 2 ** 17)
    return "chain" if chain else "exact"


def test_query_path_at_its_threshold_edges(plans):
    names = dict(zip(plans["path_names"], ("single", "chain", "exact")))
    seen = {}
    for mode, nq, n, with_q1, without_q1, one_tail, s1_split, s1_whole in plans["paths"]:
        # stage 1 as it decided before: split wherever use_filter said yes (whatever use_q1 said), else run_topk's own choice
        assert s1_split == (_path_before(mode, nq, n, single_query=False) == "chain") and s1_whole == with_q1, (mode, nq, n)
        assert names[with_q1] == _path_before(mode, nq, n), (mode, nq, n)
        assert names[without_q1] == _path_before(mode, nq, n, single_query=False), (mode, nq, n)
        # one tail: the filter chain, and one set of workspaces holds the batch (true for every size of this sweep: <= 2^29 bounds)
        assert one_tail == (names[with_q1] == "chain"), (mode, nq, n)
        seen[mode, nq, n] = names[with_q1]
    # every edge from both sides, for every mode and batch size
    for mode in range(4):
        for nq in (1, 2, 8, 9, 16, 17, 64):
            for e in (0, 2 ** 17 // nq, 400000 // nq, 800000 // nq, 50000):
                assert (mode, nq, e) in seen and (mode, nq, e + 1) in seen and (e == 0 or (mode, nq, e - 1) in seen)
    # the table itself, where the rules meet (auto mode unless said)
    assert seen[0, 1, 50001] == "single" and seen[1, 1, 50001] == "exact" and seen[2, 1, 50001] == "chain"     # one query: always the single-query kernel in auto
    assert seen[0, 8, 100000] == "single" and seen[0, 8, 100001] == "chain"                                      # nq <= 8: up to 800 000 pairs
    assert seen[0, 9, 44444] == "single" and seen[0, 9, 44445] == "chain"                                        # 9 .. 16: up to 400 000
    assert seen[0, 16, 25000] == "single" and seen[0, 16, 25001] == "chain" and seen[3, 16, 50001] == "single"   # mode 3: wherever it applies
    assert seen[0, 17, 7710] == "exact" and seen[0, 17, 7711] == "chain"                                         # 17 * 7711 >= 2^17
    assert seen[0, 64, 2047] == "exact" and seen[0, 64, 2048] == "chain" and seen[3, 64, 2047] == "exact"
    assert seen[2, 64, 0] == "exact" and seen[2, 64, 1] == "chain" and seen[1, 64, 50001] == "exact"             # nothing to filter / forced / off


def test_stage1_share_is_the_clamped_ceiling(plans):
    assert [w for w, _ in plans["share"]] == list(range(1, 65))
    for world, share in plans["share"]:
        assert share == min(128, max(8, -(-160 // world))), world
    assert dict(map(tuple, plans["share"]))[1] == 128 and dict(map(tuple, plans["share"]))[2] == 80 and dict(map(tuple, plans["share"]))[64] == 8


def test_padded_ld_is_what_filter_batch_sizes_by(plans):
    ld = dict(map(tuple, plans["ld"]))
    for n, got in ld.items():
        assert got == (n + 31) // 32 * 32 and got % 32 == 0 and 0 <= got - n < 32
    for n, nq, qb in plans["batches"]:
        if qb < nq:
            assert qb * ld[n] <= 2 ** 29 or qb == 64, (n, nq, qb)
