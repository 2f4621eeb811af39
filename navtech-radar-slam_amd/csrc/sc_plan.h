// sc_plan.h -- how a query batch is cut up and which kernels score it: the pieces of the host-buffer entry, the batches of the
// filter workspaces, the choice between the single-query kernel, the filter chain and exact-all, a shard's share of the indices
// and the XCD-aware work split of sc_spec2_filter_kernel.  Pure integer functions without a device or library dependency, so that
// tests/test_plan_logic.py can compile them with the host compiler and check their invariants (every query in exactly one
// piece / batch / workgroup) over a sweep of sizes.
#pragma once
#include <cstdint>

namespace rsx {
namespace sc {
namespace plan {

// Pieces of rsx_sc_query (sc_api.cpp): the first piece `first` queries (its upload is the only one nothing hides), every later
// one growth_x10 / 10 times the one before, multiples of 64; a remainder smaller than half a piece joins the piece before it,
// the last of max_pieces slots takes what is left.  Batches below 4 x first stay whole (first <= 0: always).  -> number of pieces
inline int host_pieces(int32_t nq, int first, int growth_x10, int max_pieces, int32_t *sizes) {
  if (growth_x10 < 10) growth_x10 = 10;
  if (first <= 0 || nq < 4 * (int64_t)first || max_pieces < 2) {
    sizes[0] = nq;
    return 1;
  }
  int n = 0;
  int32_t left = nq;
  double want = first;
  while (left > 0) {
    int32_t take = ((int32_t)want + 63) / 64 * 64;
    if (n == max_pieces - 1 || left - take < take / 2) take = left;
    sizes[n++] = take;
    left -= take;
    want *= growth_x10 / 10.0;
  }
  return n;
}

// Leading dimension of a row of bounds over n entries: whole tiles of 32 (the filter images are tile-major)
inline int64_t padded_ld(int64_t n) { return (n + 31) / 32 * 32; }

// How many of the global indices [0, n) shard `rank` of `world` owns (index % world == rank)
inline int64_t owned_below(int64_t n, int64_t rank, int64_t world) { return n > rank ? (n - rank + world - 1) / world : 0; }

// Query batch the filter workspaces are sized for: <= 2^29 bound elements (1 GiB of fp16) per batch, at least 64 queries, and
// the batches of one call equally long (8192 queries against 100 000 entries used to run as 3 x 2684 + 140)
inline int64_t filter_batch(int64_t n_items, int64_t nq) {
  const int64_t ld = padded_ld(n_items);
  int64_t qb = ld > 0 ? (1ll << 29) / ld : nq;
  qb = qb < 64 ? 64 : qb / 64 * 64;  // whole multiples of 64 queries
  if (qb >= nq) return nq;
  const int64_t nb = (nq + qb - 1) / qb;
  return ((nq + nb - 1) / nb + 63) / 64 * 64;  // <= qb: qb is a multiple of 64 and >= nq / nb
}

// ---- which kernels score nq queries against n_items entries of a shard (sc_api.cpp applies the environment overrides) ----
// filter_mode (rsx_sc_params): 0 auto, 1 filter off, 2 filter forced, 3 the single-query path wherever it applies (like auto
// for everything else)
constexpr int kQ1MaxQueries = 16;  // what one launch of the single-query kernel takes (sc_kernels.h Q1_MAX_NQ)
enum class Path {
  SingleQuery,  // sc_q1.hip: one launch, builds the queries' keys and images itself
  FilterChain,  // bounds -> short list -> window previews -> exact re-scoring
  ExactAll,     // every eligible entry exactly (launch_pairs)
};

// A handful of queries (the live detector asks one at a time, PGO.cpp:561,577): ONE launch that streams the fp16 images of
// every eligible entry once, previews every pair on the matrix cores and scores the few entries the previews cannot exclude
// exactly (sc_q1.hip) -- instead of the exact-all kernel (one entry per wavefront in fp64) or the six launches of the batched
// filter chain.  filter_mode 1 / 2 keep those paths; 3 asks for this one wherever it applies.  Records are identical.
inline bool single_query_pays(int filter_mode, int32_t nq, int64_t n_items) {
  if (nq < 1 || nq > kQ1MaxQueries || !(filter_mode == 0 || filter_mode == 3)) return false;
  // every query streams the whole database again, so with several queries against a large database the batched chain (one
  // pass of the spectral filter for all of them) takes over.  Round 6 (the queries of a call share the device's 512 workgroup
  // slots, q1_grid): MI355X, top-1, us per call single-query path / filter chain -- 10 000 keyframes: 1 query 18 / 91, 2: 22 / 94,
  // 4: 27 / 94, 8: 36 / 89; 100 000: 1 query 54 / 173, 2: 71 / 175, 4: 112 / 176, 8: 187 / 191 (round 5: 8 x 10 000 55, 8 x 100 000 305)
  // 9 .. 16 queries (32 workgroups each): 10 000 keyframes 12 queries 47 / 92, 16: 53 / 87; 50 000: 8 queries 103 / 127, 12: 167 / 134, 16: 176 / 147
  return filter_mode == 3 || nq == 1 || (int64_t)nq * n_items <= (nq <= 8 ? 800000 : 400000);
}

inline bool filter_pays(int filter_mode, int32_t nq, int64_t n_items) {
  if (filter_mode == 1 || n_items <= 0) return false;
  if (filter_mode == 2) return true;
  // the filter amortises a 300-register DB tile load over the queries of a block and costs five
  // extra launches: worth it for batched queries against a sizeable DB -- and for ANY number of queries once the DB is
  // so large that scoring every entry exactly costs more than the launches (one query, MI355X, us per query
  // exact-all / filtered: 1 000 keyframes 22 / 85, 10 000: 55 / 94, 100 000: 232 / 178)
  // (a handful of queries never gets here in auto mode unless the single-query path declined them)
  if (n_items >= 50000) return true;
  return (int64_t)nq * n_items >= (1ll << 17);  // exact-all scores ~1 G pairs/s, the chain's fixed cost is ~85 us
}

// single_query: the single-query path may be taken at all (RSX_SC_Q1=0 switches it off; the two-stage protocol asks without
// it for the stages it can split)
inline Path query_path(int filter_mode, int32_t nq, int64_t n_items, bool single_query = true) {
  if (single_query && single_query_pays(filter_mode, nq, n_items)) return Path::SingleQuery;
  return filter_pays(filter_mode, nq, n_items) ? Path::FilterChain : Path::ExactAll;
}

// The whole batch goes through ONE set of filter workspaces: its stages behind the bounds can run once over all of it (the
// host entry's pieces share one tail; the two-stage protocol stops after round 0 and goes on later)
inline bool one_tail(Path p, int64_t n_items, int32_t nq) { return p == Path::FilterChain && filter_batch(n_items, nq) >= nq; }

// What stage 1 of the two-stage protocol runs, decided in one go.  split: the chain stops after round 0 and stage 2 goes on --
// wherever the filter applies and one set of workspaces holds the batch; asked without the single-query path, which has no
// second stage to leave to.  whole: the path that scores the batch completely in stage 1 where the chain is not split
struct Stage1Plan {
  bool split;
  Path whole;
};
inline Stage1Plan stage1_plan(int filter_mode, int32_t nq, int64_t n_items, bool single_query = true) {
  return Stage1Plan{one_tail(query_path(filter_mode, nq, n_items, false), n_items, nq), query_path(filter_mode, nq, n_items, single_query)};
}

// Stage 1 of the two-stage protocol scores this shard's share of the `total` lowest bounds per query over all shards
inline int32_t stage1_share(int total, int world) {
  const int share = (total + world - 1) / world;
  return share < 8 ? 8 : (share > 128 ? 128 : share);
}

// XCD-aware split of sc_spec2_filter_kernel (sc_spec.hip): nqt query tiles, ntb tile-blocks, n_cu compute units in 8 XCDs.
// on: the split is used; XCD x owns query tiles [x * nqt_x, (x + 1) * nqt_x) in sub-ranges of len tiles, workgroup b of `grid`
// belongs to XCD b % 8 and is (sub-range (b / 8) / ntb, tile-block (b / 8) % ntb).  forced_s > 0: that many sub-ranges,
// whatever the cost.
struct XcdSplit {
  bool on;
  int32_t nqt_x, len;
  unsigned grid;
};
inline XcdSplit xcd_split(int64_t nqt, int64_t ntb, int n_cu, int64_t forced_s = 0) {
  XcdSplit r{false, 0, 0, 0u};
  const int64_t nqt_x = (nqt + 7) / 8;
  if (nqt_x < 16 || n_cu % 8 != 0 || ntb < 1) return r;
  int64_t best_s = 1;
  double best_cost = 1e300;
  const int64_t slots = n_cu / 8;
  for (int64_t S = 1; S <= 64 && (S == 1 || (nqt_x + S - 1) / S >= 16); S++) {
    const int64_t len = (nqt_x + S - 1) / S, used = (nqt_x + len - 1) / len;
    const int64_t cost = ((used * ntb + slots - 1) / slots) * (len + 3);
    if ((double)cost < best_cost * 0.995) {
      best_cost = (double)cost;
      best_s = used;
    }
  }
  if (forced_s >= 1 && forced_s <= nqt_x) best_s = forced_s;
  // against the contiguous split (perfectly balanced, one start per workgroup): only where whole rounds cost <= 6 %
  const double contiguous = (double)(ntb * nqt) / (double)n_cu + 3.0;
  if (!(best_cost <= 1.06 * contiguous) && forced_s <= 0) return r;
  r.on = true;
  r.nqt_x = (int32_t)nqt_x;
  r.len = (int32_t)((nqt_x + best_s - 1) / best_s);
  const int64_t used = (nqt_x + r.len - 1) / r.len;
  r.grid = (unsigned)(8 * used * ntb);
  return r;
}

}  // namespace plan
}  // namespace sc
}  // namespace rsx
