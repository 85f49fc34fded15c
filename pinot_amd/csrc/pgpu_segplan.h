// Per-segment filter analysis of the host planner: one pass over a segment's filter program per submit, kept in
// fixed-capacity inline storage (DESIGN.md §6 "Submit scratch").  pack_query computes a SegAnalysis per segment and
// hands it to the lead-leaf decision, plan_segment and the tile-skip plan, which used to analyse the program again
// each.  No HIP type and no pgpu_segment here: the analysis reads the filter nodes and a plain view of the query's
// columns, so tests/sanitize/segplan_fuzz.cpp drives it on the CPU against the vector-based code it replaced.
//
// Capacity rule: every container below is a SmallVec, inline up to its named capacity and on the heap beyond it
// (spill, not a fall-back path): a program that exceeds a capacity runs the same code and plans exactly as one that
// does not.  A SmallVec keeps its heap block across clear(), so reused scratch allocates at most once per high-water
// mark.
#ifndef PGPU_SEGPLAN_H
#define PGPU_SEGPLAN_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "../../include/pinot_gpu.h"

namespace segplan {

// The limits of pgpu_internal.h this header plans with (pgpu_runtime.cpp asserts that they agree)
constexpr int kTileDocs = 2048;   // PGPU_WT
constexpr int kPfxPlanes = 3;     // PGPU_PFX_PLANES
constexpr int kSliceRanges = 4;   // PGPU_SLICE_RANGES
constexpr int kMaxSlots = 8;      // PGPU_MAX_SLOTS
constexpr int kMaxStage = 6;      // PGPU_MAX_STAGE
constexpr int kColFixedBit = 1;   // PGPU_COL_FIXED_BIT
constexpr int kColRaw = 3;        // PGPU_COL_RAW
constexpr int kColMv = 4;         // PGPU_COL_MV

// Inline capacities
constexpr int kKidsCap = kMaxSlots;         // top-level AND children (one filter slot each in the kernels' programs)
constexpr int kScansCap = 2 * kMaxStage;    // SCAN leaves of all children together
constexpr int kStagedCap = kMaxStage;       // staged columns
constexpr int kMaskRuns = 64;               // id runs of one MASK leaf (64 ids)
constexpr int kListRuns = 8;                // ... of one inline LIST leaf
constexpr int kRunsCap = kMaskRuns + kListRuns;  // id runs of all children together
constexpr int kNestCap = kMaxSlots;         // open AND / OR / NOT frames of convert_filter

template <class T, int N>
class SmallVec {
  static_assert(std::is_trivially_copyable<T>::value, "SmallVec moves its elements with memcpy");

 public:
  SmallVec() {}
  SmallVec(const SmallVec&) = delete;
  SmallVec& operator=(const SmallVec&) = delete;
  ~SmallVec() {
    if (p_ != inl_) free(p_);
  }
  void clear() { n_ = 0; }
  int size() const { return n_; }
  bool empty() const { return n_ == 0; }
  bool spilled() const { return p_ != inl_; }
  T* data() { return p_; }
  const T* data() const { return p_; }
  T* begin() { return p_; }
  T* end() { return p_ + n_; }
  const T* begin() const { return p_; }
  const T* end() const { return p_ + n_; }
  T& operator[](int i) { return p_[i]; }
  const T& operator[](int i) const { return p_[i]; }
  T& back() { return p_[n_ - 1]; }
  const T& back() const { return p_[n_ - 1]; }
  void push_back(const T& v) {
    if (n_ == cap_) {
      const T copy = v;  // (v may live in this vector)
      grow(cap_ * 2);
      p_[n_++] = copy;
      return;
    }
    p_[n_++] = v;
  }
  void pop_back() { --n_; }
  void resize(int n) {  // shrink, or grow with value-initialised elements
    if (n > cap_) grow(std::max(n, cap_ * 2));
    for (int i = n_; i < n; ++i) p_[i] = T();
    n_ = n;
  }
  void assign(const SmallVec& o) {
    if (o.n_ > cap_) grow(o.n_);
    if (o.n_) memcpy((void*)p_, (const void*)o.p_, sizeof(T) * (size_t)o.n_);
    n_ = o.n_;
  }
  bool contains(const T& v) const { return std::find(begin(), end(), v) != end(); }

 private:
  void grow(int cap) {
    T* q = (T*)malloc(sizeof(T) * (size_t)cap);
    if (!q) abort();
    if (n_) memcpy((void*)q, (const void*)p_, sizeof(T) * (size_t)n_);
    if (p_ != inl_) free(p_);
    p_ = q;
    cap_ = cap;
  }
  T inl_[N];
  T* p_ = inl_;
  int n_ = 0, cap_ = N;
};

// What the analysis reads of one query column of one segment (DevColumn / HostColumn)
struct ColView {
  int32_t kind = 0;  // PGPU_COL_*
  int32_t bits = 0;
  int32_t card = 0;
  bool valid = false;      // the column map names a slot of the segment
  bool sliced = false;     // a bit-sliced copy exists
  bool presence = false;   // eligible for presence rows, and not declined
  const uint32_t* inv_cards = nullptr;  // docs per dict id of the inverted index
  int32_t num_inv_cards = 0;
};

struct ProgView {
  const pgpu_filter_node* nd;
  int n;
  const ColView* cols;  // per query column
  int ncols;
  int32_t num_docs;
  bool valid_col(int qc) const { return qc >= 0 && qc < ncols && cols[qc].valid; }
};

// Walk the subtree at node i: estimated fraction of docs it keeps (uniform-id model for scans; exact bitmap and
// sorted-range cardinalities), plus the query columns of its SCAN leaves.  Returns the index past the subtree or
// -1 on malformed input.  Estimates only steer the staging decision; results never depend on them.
template <class Scans>
inline int analyze(const ProgView& v, int i, double* sel, Scans* scans) {
  if (i < 0 || i >= v.n) return -1;
  const pgpu_filter_node& x = v.nd[i];
  const double nd = std::max(1, v.num_docs);
  switch (x.op) {
    case PGPU_F_MATCH_ALL: *sel = 1.0; return i + 1;
    case PGPU_F_EMPTY: *sel = 0.0; return i + 1;
    case PGPU_F_RAW_SCAN:
    case PGPU_F_RANGE_INDEX:
      if (!v.valid_col(x.column)) return -1;
      if (v.cols[x.column].kind == kColRaw) {  // a precomputed bitmap word per lane: never staged
        *sel = 0.5;
        return i + 1;
      }
      if (x.op == PGPU_F_RAW_SCAN) return -1;
      [[fallthrough]];  // range index of a dictionary column: a dict-id range scan on the GPU
    case PGPU_F_SCAN: {
      if (!v.valid_col(x.column)) return -1;
      if (v.cols[x.column].kind == kColMv) {  // mvpred_kernel's bitmap word per lane: never staged
        *sel = 0.5;
        return i + 1;
      }
      const double card = std::max(1, v.cols[x.column].card);
      double s = x.pred == PGPU_PRED_RANGE ? std::max(0, x.hi - x.lo) / card : std::max(0, x.num_ids) / card;
      s = std::min(1.0, s);
      *sel = x.negate ? 1.0 - s : s;
      scans->push_back(x.column);
      return i + 1;
    }
    case PGPU_F_INVERTED: {
      if (!v.valid_col(x.column)) return -1;
      const ColView& h = v.cols[x.column];
      double docs = 0;
      for (int k = 0; k < x.num_ids; ++k)
        if (x.ids[k] >= 0 && x.ids[k] < h.num_inv_cards) docs += h.inv_cards[x.ids[k]];
      const double s = std::min(1.0, docs / nd);
      *sel = x.negate ? 1.0 - s : s;
      return i + 1;
    }
    case PGPU_F_SORTED: {
      double docs = 0;
      for (int k = 0; k < x.num_ids; ++k) docs += std::max(0, x.ids[2 * k + 1] - x.ids[2 * k] + 1);
      const double s = std::min(1.0, docs / nd);
      *sel = x.negate ? 1.0 - s : s;
      return i + 1;
    }
    case PGPU_F_AND_BEGIN:
    case PGPU_F_OR_BEGIN: {
      const bool is_and = x.op == PGPU_F_AND_BEGIN;
      double acc = 1.0;  // AND: product of selectivities; OR: product of (1 - s)
      int j = i + 1;
      while (j < v.n && v.nd[j].op != (is_and ? PGPU_F_AND_END : PGPU_F_OR_END)) {
        double cs;
        j = analyze(v, j, &cs, scans);
        if (j < 0 || j >= v.n || v.nd[j].op != (is_and ? PGPU_F_AND_CHILD_END : PGPU_F_OR_CHILD_END)) return -1;
        acc *= is_and ? cs : 1.0 - cs;
        ++j;
      }
      if (j >= v.n) return -1;
      *sel = is_and ? acc : 1.0 - acc;
      return j + 1;
    }
    case PGPU_F_NOT: {
      double cs;
      const int j = analyze(v, i + 1, &cs, scans);
      *sel = 1.0 - cs;
      return j;
    }
    default:
      return -1;
  }
}

// Fraction of a b-bit column's 32-B sectors that hold at least one doc when docs survive with density rho.
inline double sector_touch(double rho, int bits) {
  if (rho >= 1.0) return 1.0;
  if (rho <= 0.0) return 0.0;
  return 1.0 - std::pow(1.0 - rho, 256.0 / bits);
}
// A column is streamed (dense) when at least half of its sectors would be read anyway.
constexpr double kDenseTouch = 0.5;

struct Run {  // dict ids [a, b)
  uint64_t a, b;
};
struct PrefixRange {  // id prefixes [lo, hi)
  uint32_t lo, hi;
  bool operator<(const PrefixRange& o) const { return lo != o.lo ? lo < o.lo : hi < o.hi; }
};

// One child of the top-level AND (or the whole filter)
struct Child {
  int begin, end;            // node range [begin, end)
  double sel;                // share of docs it keeps (analyze)
  int scan_begin, scan_end;  // its SCAN leaves' query columns in SegAnalysis::scans
  bool runs_ok;              // one plain SCAN node (scan_runs); its id runs in SegAnalysis::runs
  int run_begin, run_end;
  bool dense;
};

// The top-level AND children of a segment's filter in query order, split into the dense prefix (streamed) and the
// residual rest (per candidate doc), with what the planners ask of each child
struct SegAnalysis {
  bool done = false;  // computed for this submit
  bool ok = false;    // the program is well formed
  SmallVec<Child, kKidsCap> kids;
  SmallVec<int, kScansCap> scans;
  SmallVec<Run, kRunsCap> runs;
  SmallVec<int, kKidsCap> dense_kids, resid_kids;
  SmallVec<int, kStagedCap> staged;
  double rho = 1.0, rho_dense = 1.0;
  bool residual = false;
  void reset() {
    done = ok = false;
    kids.clear();
    scans.clear();
    runs.clear();
    dense_kids.clear();
    resid_kids.clear();
    staged.clear();
    rho = rho_dense = 1.0;
    residual = false;
  }
};

// The matching dict ids [a, b) of a child that is one non-negated SCAN node (RANGE, or a set convert_filter turns
// into an inline LIST or a MASK, clamped as it clamps them) on a fixed-bit column of <= 31 bits with a bit-sliced
// copy, appended to `runs`.  False for any other child (and nothing stays appended).
template <class Runs>
inline bool scan_runs(const ProgView& v, int begin, int end, Runs& runs) {
  if (end - begin != 1) return false;
  const pgpu_filter_node& x = v.nd[begin];
  if (x.op != PGPU_F_SCAN || x.negate) return false;
  const ColView& dc = v.cols[x.column];
  if (dc.kind != kColFixedBit || !dc.sliced || dc.bits < 1 || dc.bits > 31) return false;
  if (x.pred == PGPU_PRED_RANGE) {
    const int64_t lo = std::max(0, x.lo), hi = std::min(x.hi, dc.card);
    if (hi > lo) runs.push_back(Run{(uint64_t)lo, (uint64_t)hi});
    return true;
  }
  if (x.pred != PGPU_PRED_SET || !(dc.card <= 64 || x.num_ids <= 8) || x.num_ids < 0 || (x.num_ids && !x.ids))
    return false;
  const int mark = runs.size();
  for (int j = 0; j < x.num_ids; ++j) {
    if (x.ids[j] < 0 || x.ids[j] >= dc.card) {
      runs.resize(mark);
      return false;
    }
    runs.push_back(Run{(uint64_t)x.ids[j], (uint64_t)x.ids[j] + 1});
  }
  return true;
}

// One analysis of the segment's program: false when it is malformed.
inline bool analyze_segment(const ProgView& v, SegAnalysis& a) {
  a.reset();
  a.done = true;
  if (v.n > 0) {
    double s;
    const int e = analyze(v, 0, &s, &a.scans);
    a.scans.clear();
    if (e != v.n) return false;
    auto add = [&](int b) {
      Child c{};
      c.begin = b;
      c.scan_begin = a.scans.size();
      c.end = analyze(v, b, &c.sel, &a.scans);
      c.scan_end = a.scans.size();
      a.kids.push_back(c);
      return c.end;
    };
    if (v.nd[0].op == PGPU_F_AND_BEGIN) {
      int j = 1;
      while (v.nd[j].op != PGPU_F_AND_END) j = add(j) + 1;
    } else {
      add(0);
    }
  }
  // dense prefix of the children: every scan column of a dense child is read with >= kDenseTouch sector density
  for (int k = 0; k < a.kids.size(); ++k) {
    Child& c = a.kids[k];
    bool dense = !a.residual;
    for (int j = c.scan_begin; j < c.scan_end; ++j) {
      const ColView& dc = v.cols[a.scans[j]];
      if (dense && dc.kind == kColFixedBit && sector_touch(a.rho, dc.bits) < kDenseTouch) dense = false;
    }
    c.dense = dense;
    if (dense) {
      a.dense_kids.push_back(k);
      for (int j = c.scan_begin; j < c.scan_end; ++j) {
        const int qc = a.scans[j];
        if (v.cols[qc].kind == kColFixedBit && !a.staged.contains(qc)) a.staged.push_back(qc);
      }
    } else {
      a.residual = true;
      a.resid_kids.push_back(k);
    }
    a.rho *= c.sel;
    if (dense) a.rho_dense *= c.sel;
    c.run_begin = a.runs.size();
    c.runs_ok = scan_runs(v, c.begin, c.end, a.runs);
    c.run_end = a.runs.size();
  }
  a.ok = true;
  return true;
}

// The ranges [lo, hi) of the top K bits of a `bits`-wide column's ids that the id runs [a, b) reach, merged, and the
// share of the 2^K prefixes they cover.  False when there is none or more than kSliceRanges.
inline bool prefix_ranges(const Run* runs, int nruns, int bits, int K, PrefixRange merged[kSliceRanges], int* nmerged,
                          double* covered) {
  const int sh = bits - K;
  SmallVec<PrefixRange, kMaskRuns> pr;
  for (int i = 0; i < nruns; ++i)
    pr.push_back(PrefixRange{(uint32_t)(runs[i].a >> sh), (uint32_t)(((runs[i].b - 1) >> sh) + 1)});
  std::sort(pr.begin(), pr.end());
  int n = 0;
  PrefixRange last{0, 0};
  for (const PrefixRange& r : pr) {
    if (n && r.lo <= last.hi) {
      last.hi = std::max(last.hi, r.hi);
      if (n <= kSliceRanges) merged[n - 1] = last;
    } else {
      ++n;
      last = r;
      if (n <= kSliceRanges) merged[n - 1] = last;
    }
  }
  *nmerged = n;
  if (n == 0 || n > kSliceRanges) return false;
  *covered = 0;
  for (int i = 0; i < n; ++i) *covered += merged[i].hi - merged[i].lo;
  *covered /= (double)(1ull << K);
  return true;
}

// Lead leaf of the register-direct kernel (pgpu_lead_model in pinot_gpu.h; plan_segment plans with this function).
// A top-level AND streams its first child A and gathers the later ones per candidate.  When a later child B is far
// more selective than A, streaming only the top P planes of B's column rejects 1 - 2^-P of the docs before anything
// else is read: the survivors gather B's exact id (one 128-B line each, tools/gather_policy_bench.hip), and only
// B's matches gather A.  Bytes per 2048-doc tile:
//   today   = 256 bits_A + (prefix pre-filter ? 256 PGPU_PFX_PLANES + cand covered 128 : cand 128)
//   lead(P) = 256 P + 2048 cov_P 128 + 2048 sel_B 128 (former dense scan children)
// with cand = rho_dense 2048 candidates per tile; P = bits_B makes the lead leaf exact, B is not gathered again and
// the middle term is absent.  P is one of query_kernel_rdirect's widths below bits_B, or bits_B itself up to 16.
constexpr int kLeadWidths[4] = {8, 10, 12, 16};
inline void lead_model(int bits_a, double rho_dense, int residual_kind, int num_dense_scans, int bits_b, double sel_b,
                       const Run* runs, int nruns, pgpu_lead_model_out* out) {
  memset(out, 0, sizeof(*out));
  const double cand = rho_dense * kTileDocs;
  out->today_bytes = 256.0 * bits_a;
  if (residual_kind == PGPU_LEAD_RESID_B) {  // plan_prefix's rule
    const int K = kPfxPlanes;
    PrefixRange m[kSliceRanges];
    int nm;
    double cov = 1.0;
    if (bits_b > K && prefix_ranges(runs, nruns, bits_b, K, m, &nm, &cov) && cand * 128.0 * (1.0 - cov) > 256.0 * K)
      out->today_bytes += 256.0 * K + cand * cov * 128.0;
    else
      out->today_bytes += cand * 128.0;
  } else if (residual_kind == PGPU_LEAD_RESID_OTHER) {
    out->today_bytes += cand * 128.0;
  }
  auto consider = [&](int P) {
    PrefixRange m[kSliceRanges];
    int nm;
    double cov;
    if (!prefix_ranges(runs, nruns, bits_b, P, m, &nm, &cov)) return;
    const double lead = 256.0 * P + (P < bits_b ? kTileDocs * cov * 128.0 : 0.0) +
                        kTileDocs * sel_b * 128.0 * num_dense_scans;
    // (a tie goes to the exact leaf, which gathers less than the model's line per survivor)
    if (out->planes && (P < bits_b ? lead >= out->lead_bytes : lead > out->lead_bytes)) return;
    out->planes = P;
    out->lead_bytes = lead;
    out->num_ranges = (int32_t)nm;
    for (int r = 0; r < kSliceRanges; ++r) {
      out->ranges[r][0] = r < nm ? m[r].lo : 0;
      out->ranges[r][1] = r < nm ? m[r].hi : 0;
    }
  };
  for (int P : kLeadWidths)
    if (P < bits_b) consider(P);
  if (bits_b <= 16) consider(bits_b);
}

// A segment's lead leaf (lead_model): child `kid` of the top-level AND, streamed as the top P planes of its column
struct LeadChoice {
  int kid = -1;  // -1: the segment keeps its query order
  int col = -1, bits = 0, P = 0;
  int nr = 0;
  uint32_t rng[kSliceRanges][2] = {};
  double today = 0, lead = 0;  // modelled bytes per tile
};

// lead_choice's first look, without an analysis: the program is a top-level AND of at least two children made of
// SCAN leaves on fixed-bit columns only (queries with index, bitmap or raw leaves pay one pass over their nodes)
inline bool lead_candidate(const ProgView& v) {
  if (v.n < 6 || v.nd[0].op != PGPU_F_AND_BEGIN) return false;
  for (int i = 0; i < v.n; ++i) {
    const pgpu_filter_node& x = v.nd[i];
    const bool mark = x.op == PGPU_F_AND_BEGIN || x.op == PGPU_F_AND_CHILD_END || x.op == PGPU_F_AND_END ||
                      x.op == PGPU_F_OR_BEGIN || x.op == PGPU_F_OR_CHILD_END || x.op == PGPU_F_OR_END ||
                      x.op == PGPU_F_NOT;
    if (!mark && !(x.op == PGPU_F_SCAN && x.column >= 0 && x.column < v.ncols &&
                   v.cols[x.column].kind == kColFixedBit))
      return false;
  }
  return true;
}

// The later child of the segment's top-level AND with the cheapest lead plan, when there is one: a single non-negated
// SCAN leaf (RANGE, or a set that becomes an inline LIST / MASK) on a fixed-bit column with a bit-sliced copy, every
// other child made of SCAN leaves on fixed-bit columns only (gathered per candidate doc; bitmap, index and raw leaves
// keep their place in the dense program: lead_candidate).  Not whether it pays: pack_query decides that for the
// whole query.  `a`: the segment's analysis (analyze_segment, after lead_candidate said yes).
inline bool lead_choice(const ProgView& v, const SegAnalysis& a, LeadChoice* out) {
  if (!a.ok || a.kids.size() < 2) return false;
  int bits_a = 0;
  for (int qc : a.staged) bits_a += v.cols[qc].bits;
  for (int k = 1; k < a.kids.size(); ++k) {
    const Child& c = a.kids[k];
    if (!c.runs_ok) continue;
    const pgpu_filter_node& x = v.nd[c.begin];
    const ColView& dc = v.cols[x.column];
    const bool was_dense = c.dense;
    const int kind = a.resid_kids.empty() ? PGPU_LEAD_RESID_NONE
                     : a.resid_kids.size() == 1 && a.resid_kids[0] == k ? PGPU_LEAD_RESID_B
                                                                        : PGPU_LEAD_RESID_OTHER;
    pgpu_lead_model_out m;
    lead_model(bits_a, a.rho_dense, kind, a.dense_kids.size() - (was_dense ? 1 : 0), dc.bits, c.sel,
               a.runs.data() + c.run_begin, c.run_end - c.run_begin, &m);
    if (!m.planes || (out->kid >= 0 && m.lead_bytes >= out->lead)) continue;
    out->kid = k;
    out->col = x.column;
    out->bits = dc.bits;
    out->P = m.planes;
    out->nr = m.num_ranges;
    for (int r = 0; r < kSliceRanges; ++r) out->rng[r][0] = m.ranges[r][0], out->rng[r][1] = m.ranges[r][1];
    out->today = m.today_bytes;
    out->lead = m.lead_bytes;
  }
  return out->kid >= 0;
}

// Bytes per tile a segment in query order reads more once its launch streams no prefix planes (DevParams::rd_pfx
// is one figure per launch, and a segment with a lead leaf has none): what plan_prefix's rule says they save
inline double prefix_loss(const ProgView& v, const SegAnalysis& a) {
  if (!a.ok || a.resid_kids.size() != 1) return 0;
  const Child& c = a.kids[a.resid_kids[0]];
  if (!c.runs_ok) return 0;
  const int bits = v.cols[v.nd[c.begin].column].bits, K = kPfxPlanes;
  PrefixRange m[kSliceRanges];
  int nm;
  double cov;
  if (bits <= K || !prefix_ranges(a.runs.data() + c.run_begin, c.run_end - c.run_begin, bits, K, m, &nm, &cov)) return 0;
  return std::max(0.0, a.rho_dense * kTileDocs * 128.0 * (1.0 - cov) - 256.0 * K);
}

}  // namespace segplan

#endif  // PGPU_SEGPLAN_H
