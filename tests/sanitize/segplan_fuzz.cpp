// Differential harness for pinot_amd/csrc/pgpu_segplan.h (tests/test_segplan_host.py builds it with ASan + UBSan).
//
// namespace old holds a verbatim copy of the vector-based analyze / split_children / scan_runs / prefix_ranges /
// lead_model / prefix_loss / lead_choice that pgpu_runtime.cpp planned with before the analysis moved into the
// header, over stand-ins for the runtime's structs that carry only the fields those functions read.  Every case is
// planned by both and compared field by field, doubles bit for bit.
//
//   segplan_fuzz directed            the directed cases
//   segplan_fuzz random SEED COUNT   COUNT seeded random programs (the failing case's seed is printed)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <deque>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "pgpu_segplan.h"

#define PGPU_COL_NONE 0
#define PGPU_COL_FIXED_BIT 1
#define PGPU_COL_SORTED 2
#define PGPU_COL_RAW 3
#define PGPU_COL_MV 4
#define PGPU_WT 2048
#define PGPU_PFX_PLANES 3
#define PGPU_SLICE_RANGES 4
#define PGPU_MAX_SLOTS 8
#define PGPU_MAX_STAGE 6

static_assert(segplan::kTileDocs == PGPU_WT && segplan::kPfxPlanes == PGPU_PFX_PLANES &&
              segplan::kSliceRanges == PGPU_SLICE_RANGES && segplan::kMaxSlots == PGPU_MAX_SLOTS &&
              segplan::kMaxStage == PGPU_MAX_STAGE, "limits");

namespace old {

struct DevColumn {
  int32_t kind, bits, card;
  const uint32_t* sliced;
};
struct HostColumn {
  std::vector<uint32_t> inv_cards;
};
struct pgpu_segment {
  int32_t num_docs;
  std::vector<HostColumn> cols;
  std::vector<DevColumn> dev;
};
struct pgpu_segment_plan {
  const int32_t* column_map;
};
struct pgpu_query_desc {
  int32_t num_columns;
};

struct SegView {
  const pgpu_query_desc* q;
  const pgpu_segment_plan* sp;
  const pgpu_segment* seg;
  const pgpu_filter_node* nd;
  int n;
  const HostColumn* host(int qc) const { return &seg->cols[sp->column_map[qc]]; }
  const DevColumn* dev(int qc) const { return &seg->dev[sp->column_map[qc]]; }
};

int analyze(const SegView& v, int i, double* sel, std::vector<int>* scans) {
  if (i < 0 || i >= v.n) return -1;
  const pgpu_filter_node& x = v.nd[i];
  const double nd = std::max(1, v.seg->num_docs);
  auto valid_col = [&](int qc) {
    return qc >= 0 && qc < v.q->num_columns && v.sp->column_map[qc] >= 0 &&
           v.sp->column_map[qc] < (int32_t)v.seg->dev.size();
  };
  switch (x.op) {
    case PGPU_F_MATCH_ALL: *sel = 1.0; return i + 1;
    case PGPU_F_EMPTY: *sel = 0.0; return i + 1;
    case PGPU_F_RAW_SCAN:
    case PGPU_F_RANGE_INDEX:
      if (!valid_col(x.column)) return -1;
      if (v.dev(x.column)->kind == PGPU_COL_RAW) {  // a precomputed bitmap word per lane: never staged
        *sel = 0.5;
        return i + 1;
      }
      if (x.op == PGPU_F_RAW_SCAN) return -1;
      [[fallthrough]];  // range index of a dictionary column: a dict-id range scan on the GPU
    case PGPU_F_SCAN: {
      if (!valid_col(x.column)) return -1;
      if (v.dev(x.column)->kind == PGPU_COL_MV) {  // mvpred_kernel's bitmap word per lane: never staged
        *sel = 0.5;
        return i + 1;
      }
      const double card = std::max(1, v.dev(x.column)->card);
      double s = x.pred == PGPU_PRED_RANGE ? std::max(0, x.hi - x.lo) / card : std::max(0, x.num_ids) / card;
      s = std::min(1.0, s);
      *sel = x.negate ? 1.0 - s : s;
      scans->push_back(x.column);
      return i + 1;
    }
    case PGPU_F_INVERTED: {
      if (!valid_col(x.column)) return -1;
      const HostColumn* h = v.host(x.column);
      double docs = 0;
      for (int k = 0; k < x.num_ids; ++k)
        if (x.ids[k] >= 0 && x.ids[k] < (int32_t)h->inv_cards.size()) docs += h->inv_cards[x.ids[k]];
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

double sector_touch(double rho, int bits) {
  if (rho >= 1.0) return 1.0;
  if (rho <= 0.0) return 0.0;
  return 1.0 - std::pow(1.0 - rho, 256.0 / bits);
}

constexpr double kDenseTouch = 0.5;

bool prefix_ranges(const std::vector<std::pair<uint64_t, uint64_t>>& runs, int bits, int K,
                   std::vector<std::pair<uint32_t, uint32_t>>& merged, double* covered) {
  const int sh = bits - K;
  std::vector<std::pair<uint32_t, uint32_t>> pr;
  for (auto& r : runs) pr.emplace_back((uint32_t)(r.first >> sh), (uint32_t)(((r.second - 1) >> sh) + 1));
  std::sort(pr.begin(), pr.end());
  merged.clear();
  for (auto& r : pr) {
    if (!merged.empty() && r.first <= merged.back().second) merged.back().second = std::max(merged.back().second, r.second);
    else merged.push_back(r);
  }
  if (merged.empty() || (int)merged.size() > PGPU_SLICE_RANGES) return false;
  *covered = 0;
  for (auto& r : merged) *covered += r.second - r.first;
  *covered /= (double)(1ull << K);
  return true;
}

constexpr int kLeadWidths[4] = {8, 10, 12, 16};
void lead_model(int bits_a, double rho_dense, int residual_kind, int num_dense_scans, int bits_b, double sel_b,
                const std::vector<std::pair<uint64_t, uint64_t>>& runs, pgpu_lead_model_out* out) {
  memset(out, 0, sizeof(*out));
  const double cand = rho_dense * PGPU_WT;
  out->today_bytes = 256.0 * bits_a;
  if (residual_kind == PGPU_LEAD_RESID_B) {  // plan_prefix's rule
    const int K = PGPU_PFX_PLANES;
    std::vector<std::pair<uint32_t, uint32_t>> m;
    double cov = 1.0;
    if (bits_b > K && prefix_ranges(runs, bits_b, K, m, &cov) && cand * 128.0 * (1.0 - cov) > 256.0 * K)
      out->today_bytes += 256.0 * K + cand * cov * 128.0;
    else
      out->today_bytes += cand * 128.0;
  } else if (residual_kind == PGPU_LEAD_RESID_OTHER) {
    out->today_bytes += cand * 128.0;
  }
  auto consider = [&](int P) {
    std::vector<std::pair<uint32_t, uint32_t>> m;
    double cov;
    if (!prefix_ranges(runs, bits_b, P, m, &cov)) return;
    const double lead = 256.0 * P + (P < bits_b ? PGPU_WT * cov * 128.0 : 0.0) +
                        PGPU_WT * sel_b * 128.0 * num_dense_scans;
    // (a tie goes to the exact leaf, which gathers less than the model's line per survivor)
    if (out->planes && (P < bits_b ? lead >= out->lead_bytes : lead > out->lead_bytes)) return;
    out->planes = P;
    out->lead_bytes = lead;
    out->num_ranges = (int32_t)m.size();
    for (int r = 0; r < PGPU_SLICE_RANGES; ++r) {
      out->ranges[r][0] = r < (int)m.size() ? m[r].first : 0;
      out->ranges[r][1] = r < (int)m.size() ? m[r].second : 0;
    }
  };
  for (int P : kLeadWidths)
    if (P < bits_b) consider(P);
  if (bits_b <= 16) consider(bits_b);
}

struct ChildSplit {
  std::vector<std::pair<int, int>> kids;  // node ranges [begin, end)
  std::vector<double> sel;                // share of docs each child keeps (analyze)
  std::vector<int> dense_kids, resid_kids, staged;
  double rho = 1.0, rho_dense = 1.0;
  bool residual = false;
};
bool split_children(const SegView& v, ChildSplit& cs) {
  std::vector<std::pair<int, int>>& kids = cs.kids;
  if (v.n > 0) {
    double s;
    std::vector<int> scans;
    const int e = analyze(v, 0, &s, &scans);
    if (e != v.n) return false;
    if (v.nd[0].op == PGPU_F_AND_BEGIN) {
      int j = 1;
      while (v.nd[j].op != PGPU_F_AND_END) {
        const int ce = analyze(v, j, &s, &scans);
        kids.emplace_back(j, ce);
        j = ce + 1;
      }
    } else {
      kids.emplace_back(0, v.n);
    }
  }
  // dense prefix of the children: every scan column of a dense child is read with >= kDenseTouch sector density
  for (size_t k = 0; k < kids.size(); ++k) {
    double s;
    std::vector<int> scans;
    analyze(v, kids[k].first, &s, &scans);
    bool dense = !cs.residual;
    for (int qc : scans)
      if (dense && v.dev(qc)->kind == PGPU_COL_FIXED_BIT && sector_touch(cs.rho, v.dev(qc)->bits) < kDenseTouch)
        dense = false;
    if (dense) {
      cs.dense_kids.push_back((int)k);
      for (int qc : scans)
        if (v.dev(qc)->kind == PGPU_COL_FIXED_BIT && std::find(cs.staged.begin(), cs.staged.end(), qc) == cs.staged.end())
          cs.staged.push_back(qc);
    } else {
      cs.residual = true;
      cs.resid_kids.push_back((int)k);
    }
    cs.sel.push_back(s);
    cs.rho *= s;
    if (dense) cs.rho_dense *= s;
  }
  return true;
}

struct LeadChoice {
  int kid = -1;  // -1: the segment keeps its query order
  int col = -1, bits = 0, P = 0;
  int nr = 0;
  uint32_t rng[PGPU_SLICE_RANGES][2] = {};
  double today = 0, lead = 0;  // modelled bytes per tile
};

bool scan_runs(const SegView& v, const std::pair<int, int>& kid, std::vector<std::pair<uint64_t, uint64_t>>& runs) {
  if (kid.second - kid.first != 1) return false;
  const pgpu_filter_node& x = v.nd[kid.first];
  if (x.op != PGPU_F_SCAN || x.negate) return false;
  const DevColumn* dc = v.dev(x.column);
  if (dc->kind != PGPU_COL_FIXED_BIT || !dc->sliced || dc->bits < 1 || dc->bits > 31) return false;
  if (x.pred == PGPU_PRED_RANGE) {
    const int64_t lo = std::max(0, x.lo), hi = std::min(x.hi, dc->card);
    if (hi > lo) runs.emplace_back((uint64_t)lo, (uint64_t)hi);
    return true;
  }
  if (x.pred != PGPU_PRED_SET || !(dc->card <= 64 || x.num_ids <= 8) || x.num_ids < 0 || (x.num_ids && !x.ids))
    return false;
  for (int j = 0; j < x.num_ids; ++j) {
    if (x.ids[j] < 0 || x.ids[j] >= dc->card) return false;
    runs.emplace_back((uint64_t)x.ids[j], (uint64_t)x.ids[j] + 1);
  }
  return true;
}

double prefix_loss(const SegView& v) {
  ChildSplit cs;
  std::vector<std::pair<uint64_t, uint64_t>> runs;
  if (!split_children(v, cs) || cs.resid_kids.size() != 1 || !scan_runs(v, cs.kids[cs.resid_kids[0]], runs)) return 0;
  const int bits = v.dev(v.nd[cs.kids[cs.resid_kids[0]].first].column)->bits, K = PGPU_PFX_PLANES;
  std::vector<std::pair<uint32_t, uint32_t>> m;
  double cov;
  if (bits <= K || !prefix_ranges(runs, bits, K, m, &cov)) return 0;
  return std::max(0.0, cs.rho_dense * PGPU_WT * 128.0 * (1.0 - cov) - 256.0 * K);
}

bool lead_choice(const SegView& v, LeadChoice* out) {
  if (v.n < 6 || v.nd[0].op != PGPU_F_AND_BEGIN) return false;
  // (first, and without the analysis below: queries with index, bitmap or raw leaves pay one pass over their nodes)
  for (int i = 0; i < v.n; ++i) {
    const pgpu_filter_node& x = v.nd[i];
    const bool mark = x.op == PGPU_F_AND_BEGIN || x.op == PGPU_F_AND_CHILD_END || x.op == PGPU_F_AND_END ||
                      x.op == PGPU_F_OR_BEGIN || x.op == PGPU_F_OR_CHILD_END || x.op == PGPU_F_OR_END ||
                      x.op == PGPU_F_NOT;
    if (!mark && !(x.op == PGPU_F_SCAN && x.column >= 0 && x.column < v.q->num_columns &&
                   v.dev(x.column)->kind == PGPU_COL_FIXED_BIT))
      return false;
  }
  ChildSplit cs;
  if (!split_children(v, cs) || cs.kids.size() < 2) return false;
  int bits_a = 0;
  for (int qc : cs.staged) bits_a += v.dev(qc)->bits;
  for (size_t k = 1; k < cs.kids.size(); ++k) {
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    if (!scan_runs(v, cs.kids[k], runs)) continue;
    const pgpu_filter_node& x = v.nd[cs.kids[k].first];
    const DevColumn* dc = v.dev(x.column);
    const bool was_dense = std::find(cs.dense_kids.begin(), cs.dense_kids.end(), (int)k) != cs.dense_kids.end();
    const int kind = cs.resid_kids.empty() ? PGPU_LEAD_RESID_NONE
                     : cs.resid_kids.size() == 1 && cs.resid_kids[0] == (int)k ? PGPU_LEAD_RESID_B
                                                                                : PGPU_LEAD_RESID_OTHER;
    pgpu_lead_model_out m;
    lead_model(bits_a, cs.rho_dense, kind, (int)cs.dense_kids.size() - (was_dense ? 1 : 0), dc->bits, cs.sel[k], runs, &m);
    if (!m.planes || (out->kid >= 0 && m.lead_bytes >= out->lead)) continue;
    out->kid = (int)k;
    out->col = x.column;
    out->bits = dc->bits;
    out->P = m.planes;
    out->nr = m.num_ranges;
    for (int r = 0; r < PGPU_SLICE_RANGES; ++r) out->rng[r][0] = m.ranges[r][0], out->rng[r][1] = m.ranges[r][1];
    out->today = m.today_bytes;
    out->lead = m.lead_bytes;
  }
  return out->kid >= 0;
}

}  // namespace old

namespace {

struct Col {
  int32_t kind, bits, card;
  bool sliced;
  std::vector<uint32_t> inv_cards;
};

struct Case {
  std::string name;
  std::vector<Col> cols;
  int32_t num_docs = 6161;
  std::vector<pgpu_filter_node> nodes;
  std::deque<std::vector<int32_t>> ids;  // (a deque: the nodes point into its elements)

  int col(int kind, int bits, int card, bool sliced = true) {
    Col c{kind, bits, card, sliced, {}};
    cols.push_back(c);
    return (int)cols.size() - 1;
  }
  void mark(int op) {
    pgpu_filter_node nd;
    memset(&nd, 0, sizeof(nd));
    nd.op = op;
    nodes.push_back(nd);
  }
  void range(int c, int lo, int hi, int negate = 0, int op = PGPU_F_SCAN) {
    pgpu_filter_node nd;
    memset(&nd, 0, sizeof(nd));
    nd.op = op;
    nd.column = c;
    nd.pred = PGPU_PRED_RANGE;
    nd.lo = lo;
    nd.hi = hi;
    nd.negate = negate;
    nodes.push_back(nd);
  }
  void set(int c, const std::vector<int32_t>& v, int negate = 0, int op = PGPU_F_SCAN) {
    ids.push_back(v);
    pgpu_filter_node nd;
    memset(&nd, 0, sizeof(nd));
    nd.op = op;
    nd.column = c;
    nd.pred = PGPU_PRED_SET;
    nd.negate = negate;
    nd.ids = ids.back().empty() ? nullptr : ids.back().data();
    nd.num_ids = op == PGPU_F_SORTED ? (int)v.size() / 2 : (int)v.size();
    nodes.push_back(nd);
  }
};

int failures = 0;
#define CHECK(cond, what)                                                              \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      fprintf(stderr, "MISMATCH %s: %s (line %d)\n", c.name.c_str(), what, __LINE__);  \
      ++failures;                                                                      \
      return false;                                                                    \
    }                                                                                  \
  } while (0)

bool same(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

bool same_model(const pgpu_lead_model_out& a, const pgpu_lead_model_out& b) {
  return a.planes == b.planes && a.num_ranges == b.num_ranges && memcmp(a.ranges, b.ranges, sizeof(a.ranges)) == 0 &&
         same(a.today_bytes, b.today_bytes) && same(a.lead_bytes, b.lead_bytes);
}

// Plan the case with both and compare.  expect_ok: < 0 do not care, else whether the program must be accepted.
bool check(const Case& c, int expect_ok = -1) {
  const int ncols = (int)c.cols.size();
  std::vector<int32_t> cmap(ncols);
  old::pgpu_segment seg;
  seg.num_docs = c.num_docs;
  static const uint32_t plane = 0;
  std::vector<segplan::ColView> view(ncols);
  for (int i = 0; i < ncols; ++i) {
    cmap[i] = ncols - 1 - i;  // (a column map that is not the identity)
  }
  seg.cols.resize(ncols);
  seg.dev.resize(ncols);
  for (int i = 0; i < ncols; ++i) {
    const Col& k = c.cols[i];
    seg.dev[cmap[i]] = old::DevColumn{k.kind, k.bits, k.card, k.sliced ? &plane : nullptr};
    seg.cols[cmap[i]].inv_cards = k.inv_cards;
  }
  for (int i = 0; i < ncols; ++i) {
    const Col& k = c.cols[i];
    segplan::ColView& cv = view[i];
    cv.kind = k.kind;
    cv.bits = k.bits;
    cv.card = k.card;
    cv.valid = true;
    cv.sliced = k.sliced;
    cv.inv_cards = seg.cols[cmap[i]].inv_cards.data();
    cv.num_inv_cards = (int32_t)seg.cols[cmap[i]].inv_cards.size();
  }
  old::pgpu_segment_plan sp{cmap.data()};
  old::pgpu_query_desc q{ncols};
  old::SegView ov{&q, &sp, &seg, c.nodes.data(), (int)c.nodes.size()};
  segplan::ProgView nv{c.nodes.data(), (int)c.nodes.size(), view.data(), ncols, c.num_docs};

  old::ChildSplit cs;
  const bool ook = old::split_children(ov, cs);
  segplan::SegAnalysis a;
  const bool nok = segplan::analyze_segment(nv, a);
  CHECK(ook == nok, "accepted");
  CHECK(a.done && a.ok == nok, "flags");
  if (expect_ok >= 0) CHECK(nok == (expect_ok != 0), "expected acceptance");
  if (nok) {
    CHECK((int)cs.kids.size() == a.kids.size(), "kids");
    for (int k = 0; k < a.kids.size(); ++k) {
      CHECK(cs.kids[k].first == a.kids[k].begin && cs.kids[k].second == a.kids[k].end, "kid range");
      CHECK(same(cs.sel[k], a.kids[k].sel), "kid sel");
      const bool od = std::find(cs.dense_kids.begin(), cs.dense_kids.end(), k) != cs.dense_kids.end();
      CHECK(od == a.kids[k].dense, "kid dense");
      std::vector<int> oscans;
      double s;
      old::analyze(ov, cs.kids[k].first, &s, &oscans);
      CHECK((int)oscans.size() == a.kids[k].scan_end - a.kids[k].scan_begin, "kid scans");
      for (size_t j = 0; j < oscans.size(); ++j) CHECK(oscans[j] == a.scans[a.kids[k].scan_begin + (int)j], "kid scan col");
      std::vector<std::pair<uint64_t, uint64_t>> oruns;
      const bool ork = old::scan_runs(ov, cs.kids[k], oruns);
      CHECK(ork == a.kids[k].runs_ok, "runs ok");
      const int nr = a.kids[k].run_end - a.kids[k].run_begin;
      if (!ork) {
        CHECK(nr == 0, "runs of a rejected child");
        continue;
      }
      CHECK((int)oruns.size() == nr, "runs");
      const segplan::Run* runs = a.runs.data() + a.kids[k].run_begin;
      for (int j = 0; j < nr; ++j) CHECK(oruns[j].first == runs[j].a && oruns[j].second == runs[j].b, "run");
      const int bits = c.cols[c.nodes[a.kids[k].begin].column].bits;
      for (int K : {3, 8, 10, 12, 16, bits}) {
        if (K > bits) continue;
        std::vector<std::pair<uint32_t, uint32_t>> om;
        double ocov = -1, ncov = -1;
        segplan::PrefixRange nm[segplan::kSliceRanges];
        int nn = 0;
        const bool op = old::prefix_ranges(oruns, bits, K, om, &ocov);
        const bool np = segplan::prefix_ranges(runs, nr, bits, K, nm, &nn, &ncov);
        CHECK(op == np, "prefix ok");
        CHECK((int)om.size() == nn, "prefix count");
        if (!op) continue;
        CHECK(same(ocov, ncov), "prefix covered");
        for (int j = 0; j < nn; ++j) CHECK(om[j].first == nm[j].lo && om[j].second == nm[j].hi, "prefix range");
      }
      for (int kind = PGPU_LEAD_RESID_NONE; kind <= PGPU_LEAD_RESID_OTHER; ++kind) {
        pgpu_lead_model_out mo, mn;
        old::lead_model(17 + k, cs.rho_dense, kind, k, bits, cs.sel[k], oruns, &mo);
        segplan::lead_model(17 + k, a.rho_dense, kind, k, bits, a.kids[k].sel, runs, nr, &mn);
        CHECK(same_model(mo, mn), "lead model");
      }
    }
    auto same_list = [](const std::vector<int>& o, const auto& n) {
      if ((int)o.size() != n.size()) return false;
      for (int j = 0; j < n.size(); ++j)
        if (o[j] != n[j]) return false;
      return true;
    };
    CHECK(same_list(cs.dense_kids, a.dense_kids), "dense kids");
    CHECK(same_list(cs.resid_kids, a.resid_kids), "residual kids");
    CHECK(same_list(cs.staged, a.staged), "staged");
    CHECK(same(cs.rho, a.rho) && same(cs.rho_dense, a.rho_dense), "rho");
    CHECK(cs.residual == a.residual, "residual");
  }
  old::LeadChoice ol;
  segplan::LeadChoice nl;
  const bool olc = old::lead_choice(ov, &ol);
  const bool nlc = segplan::lead_candidate(nv) && segplan::lead_choice(nv, a, &nl);
  CHECK(olc == nlc, "lead choice");
  if (olc) {
    CHECK(ol.kid == nl.kid && ol.col == nl.col && ol.bits == nl.bits && ol.P == nl.P && ol.nr == nl.nr, "lead fields");
    CHECK(memcmp(ol.rng, nl.rng, sizeof(ol.rng)) == 0, "lead ranges");
    CHECK(same(ol.today, nl.today) && same(ol.lead, nl.lead), "lead bytes");
  }
  CHECK(same(old::prefix_loss(ov), segplan::prefix_loss(nv, a)), "prefix loss");
  return true;
}

// ---- directed cases -------------------------------------------------------------------------------------------

// a top-level AND of n range children over n fixed-bit columns (every child dense: wide ranges)
Case and_of(int n, const char* what) {
  Case c;
  c.name = std::string(what) + " x" + std::to_string(n);
  for (int i = 0; i < n; ++i) c.col(PGPU_COL_FIXED_BIT, 4 + i % 5, 10 + i);
  if (n > 1) c.mark(PGPU_F_AND_BEGIN);
  for (int i = 0; i < n; ++i) {
    c.range(i, 0, 9 + i);
    if (n > 1) c.mark(PGPU_F_AND_CHILD_END);
  }
  if (n > 1) c.mark(PGPU_F_AND_END);
  return c;
}

void directed() {
  using namespace segplan;
  // children / staged columns at every inline capacity
  for (int cap : {kKidsCap, kStagedCap, kScansCap})
    for (int n : {1, 2, cap - 1, cap, cap + 1}) check(and_of(n, "and"), 1);
  // SCAN leaves of all children together at kScansCap: children that are ORs of two scans
  for (int n : {kScansCap / 2 - 1, kScansCap / 2, kScansCap / 2 + 1}) {
    Case c;
    c.name = "or-children x" + std::to_string(n);
    for (int i = 0; i < 2 * n; ++i) c.col(PGPU_COL_FIXED_BIT, 6, 50);
    c.mark(PGPU_F_AND_BEGIN);
    for (int i = 0; i < n; ++i) {
      c.mark(PGPU_F_OR_BEGIN);
      c.range(2 * i, 0, 40);
      c.mark(PGPU_F_OR_CHILD_END);
      c.range(2 * i + 1, 3, 45);
      c.mark(PGPU_F_OR_CHILD_END);
      c.mark(PGPU_F_OR_END);
      c.mark(PGPU_F_AND_CHILD_END);
    }
    c.mark(PGPU_F_AND_END);
    check(c, 1);
  }
  // id runs of all children together at kRunsCap: MASK leaves of 32 runs each, and LIST leaves of 8
  for (int total : {kRunsCap - 1, kRunsCap, kRunsCap + 1}) {
    Case c;
    c.name = "runs x" + std::to_string(total);
    c.mark(PGPU_F_AND_BEGIN);
    int left = total, i = 0;
    while (left > 0) {
      const int take = std::min(left, 32);
      c.col(PGPU_COL_FIXED_BIT, 6, 64);
      std::vector<int32_t> v;
      for (int j = 0; j < take; ++j) v.push_back(2 * j);
      c.set(i++, v);
      c.mark(PGPU_F_AND_CHILD_END);
      left -= take;
    }
    c.col(PGPU_COL_FIXED_BIT, 20, 1 << 20);
    c.range(i, 5, 6);
    c.mark(PGPU_F_AND_CHILD_END);
    c.mark(PGPU_F_AND_END);
    check(c, 1);
  }
  // nesting at PGPU_MAX_SLOTS - 2 and - 1 (alternating AND / OR, one leaf at the bottom), beside a second child
  for (int depth : {kMaxSlots - 2, kMaxSlots - 1}) {
    Case c;
    c.name = "nest " + std::to_string(depth);
    c.col(PGPU_COL_FIXED_BIT, 10, 1000);
    c.col(PGPU_COL_FIXED_BIT, 20, 1 << 20);
    for (int d = 0; d < depth; ++d) c.mark(d % 2 ? PGPU_F_OR_BEGIN : PGPU_F_AND_BEGIN);
    c.range(0, 10, 700);
    for (int d = depth - 1; d >= 0; --d) {
      c.mark(d % 2 ? PGPU_F_OR_CHILD_END : PGPU_F_AND_CHILD_END);
      if (d == 0) {
        c.set(1, {77});
        c.mark(PGPU_F_AND_CHILD_END);
      }
      c.mark(d % 2 ? PGPU_F_OR_END : PGPU_F_AND_END);
    }
    check(c, 1);
  }
  // an OR and a NOT as a child
  {
    Case c;
    c.name = "or + not children";
    c.col(PGPU_COL_FIXED_BIT, 10, 1000);
    c.col(PGPU_COL_FIXED_BIT, 20, 1 << 20);
    c.col(PGPU_COL_FIXED_BIT, 6, 40);
    c.mark(PGPU_F_AND_BEGIN);
    c.mark(PGPU_F_OR_BEGIN);
    c.range(0, 10, 700);
    c.mark(PGPU_F_OR_CHILD_END);
    c.set(2, {1, 5});
    c.mark(PGPU_F_OR_CHILD_END);
    c.mark(PGPU_F_OR_END);
    c.mark(PGPU_F_AND_CHILD_END);
    c.mark(PGPU_F_NOT);
    c.set(1, {4, 9, 1000});
    c.mark(PGPU_F_AND_CHILD_END);
    c.set(1, {123456});
    c.mark(PGPU_F_AND_CHILD_END);
    c.mark(PGPU_F_AND_END);
    check(c, 1);
  }
  // IN lists of 0, 1, 8 and 9 ids on a wide column, alone and behind a dense range
  for (int n : {0, 1, 8, 9})
    for (int with_range : {0, 1}) {
      Case c;
      c.name = "in x" + std::to_string(n) + (with_range ? " behind a range" : "");
      c.col(PGPU_COL_FIXED_BIT, 6, 60);
      c.col(PGPU_COL_FIXED_BIT, 20, 1 << 20);
      std::vector<int32_t> v;
      for (int j = 0; j < n; ++j) v.push_back(1000 + 70001 * j);
      if (with_range) {
        c.mark(PGPU_F_AND_BEGIN);
        c.range(0, 0, 30);
        c.mark(PGPU_F_AND_CHILD_END);
      }
      c.set(1, v);
      if (with_range) {
        c.mark(PGPU_F_AND_CHILD_END);
        c.mark(PGPU_F_AND_END);
      }
      check(c, 1);
    }
  // MASK leaves: 64 ids' alternating bits (32 runs), 4 and 5 runs; an id out of range; a duplicate id
  {
    std::vector<std::vector<int32_t>> sets;
    std::vector<int32_t> alt;
    for (int j = 0; j < 64; j += 2) alt.push_back(j);
    sets.push_back(alt);
    sets.push_back({1, 2, 3, 10, 11, 30, 31, 32, 60});
    sets.push_back({1, 2, 3, 10, 11, 30, 31, 32, 60, 63});
    sets.push_back({1, 64});
    sets.push_back({5, 5, 6});
    for (size_t k = 0; k < sets.size(); ++k) {
      Case c;
      c.name = "mask " + std::to_string(k);
      c.col(PGPU_COL_FIXED_BIT, 12, 3000);
      c.col(PGPU_COL_FIXED_BIT, 6, 64);
      c.mark(PGPU_F_AND_BEGIN);
      c.range(0, 0, 2500);
      c.mark(PGPU_F_AND_CHILD_END);
      c.set(1, sets[k]);
      c.mark(PGPU_F_AND_CHILD_END);
      c.mark(PGPU_F_AND_END);
      check(c, 1);
    }
  }
  // ids whose prefixes fall into exactly PGPU_SLICE_RANGES and PGPU_SLICE_RANGES + 1 ranges at each lead width
  for (int P : {8, 10, 12, 16})
    for (int n : {kSliceRanges, kSliceRanges + 1})
      for (int bits : {P, P + 4, 31}) {
        if (bits < P) continue;
        Case c;
        c.name = "prefixes P" + std::to_string(P) + " n" + std::to_string(n) + " bits" + std::to_string(bits);
        c.col(PGPU_COL_FIXED_BIT, 8, 200);
        c.col(PGPU_COL_FIXED_BIT, bits, (int32_t)std::min<int64_t>(INT32_MAX, 1ll << bits));
        std::vector<int32_t> v;
        for (int j = 0; j < n; ++j) v.push_back((int32_t)(((int64_t)(2 * j + 1) << (bits - P)) + (j & 1)));
        c.mark(PGPU_F_AND_BEGIN);
        c.range(0, 0, 150);
        c.mark(PGPU_F_AND_CHILD_END);
        c.set(1, v);
        c.mark(PGPU_F_AND_CHILD_END);
        c.mark(PGPU_F_AND_END);
        check(c, 1);
      }
  // a range clamped by card, an empty range, a negative bound, a negated range
  for (int k = 0; k < 4; ++k) {
    Case c;
    c.name = "range " + std::to_string(k);
    c.col(PGPU_COL_FIXED_BIT, 8, 200);
    c.col(PGPU_COL_FIXED_BIT, 20, 777777);
    c.mark(PGPU_F_AND_BEGIN);
    c.range(0, 0, 150);
    c.mark(PGPU_F_AND_CHILD_END);
    if (k == 0) c.range(1, 777000, 900000);
    if (k == 1) c.range(1, 500, 500);
    if (k == 2) c.range(1, -5, 3);
    if (k == 3) c.range(1, 10, 12, 1);
    c.mark(PGPU_F_AND_CHILD_END);
    c.mark(PGPU_F_AND_END);
    check(c, 1);
  }
  // a column without a bit-sliced copy; 32 bits; a selective first child (the second turns residual)
  for (int k = 0; k < 3; ++k) {
    Case c;
    c.name = "columns " + std::to_string(k);
    c.col(PGPU_COL_FIXED_BIT, 16, 60000);
    c.col(PGPU_COL_FIXED_BIT, k == 1 ? 32 : 20, 1 << 20, k != 0);
    c.mark(PGPU_F_AND_BEGIN);
    c.range(0, 0, k == 2 ? 20 : 50000);
    c.mark(PGPU_F_AND_CHILD_END);
    c.set(1, {4242});
    c.mark(PGPU_F_AND_CHILD_END);
    c.mark(PGPU_F_AND_END);
    check(c, 1);
  }
  // INVERTED and SORTED leaves, a raw scan, a range index and a multi-value scan beside SCAN leaves
  {
    Case c;
    c.name = "index leaves";
    const int f = c.col(PGPU_COL_FIXED_BIT, 10, 1000);
    const int inv = c.col(PGPU_COL_FIXED_BIT, 8, 5);
    c.cols[inv].inv_cards = {100, 2000, 0, 61, 4000};
    const int srt = c.col(PGPU_COL_SORTED, 0, 30);
    const int raw = c.col(PGPU_COL_RAW, 0, 0, false);
    const int mv = c.col(PGPU_COL_MV, 7, 100, false);
    c.mark(PGPU_F_AND_BEGIN);
    c.set(srt, {0, 99, 200, 150, 300, 6160}, 0, PGPU_F_SORTED);
    c.mark(PGPU_F_AND_CHILD_END);
    c.set(inv, {0, 3, 7, -1}, 1, PGPU_F_INVERTED);
    c.mark(PGPU_F_AND_CHILD_END);
    c.range(raw, 0, 0, 0, PGPU_F_RAW_SCAN);
    c.mark(PGPU_F_AND_CHILD_END);
    c.range(f, 100, 900, 0, PGPU_F_RANGE_INDEX);
    c.mark(PGPU_F_AND_CHILD_END);
    c.set(mv, {1, 2});
    c.mark(PGPU_F_AND_CHILD_END);
    c.set(f, {5, 6, 900});
    c.mark(PGPU_F_AND_CHILD_END);
    c.mark(PGPU_F_AND_END);
    check(c, 1);
  }
  // no filter, MATCH_ALL, EMPTY
  {
    Case c;
    c.name = "no filter";
    c.col(PGPU_COL_FIXED_BIT, 10, 1000);
    check(c, 1);
    c.name = "match all";
    c.mark(PGPU_F_MATCH_ALL);
    check(c, 1);
    c.nodes.clear();
    c.name = "empty";
    c.mark(PGPU_F_EMPTY);
    check(c, 1);
  }
  // malformed programs: each is rejected
  {
    Case base;
    base.col(PGPU_COL_FIXED_BIT, 10, 1000);
    base.col(PGPU_COL_FIXED_BIT, 20, 1 << 20);
    {
      Case c = base;
      c.name = "unterminated AND";
      c.mark(PGPU_F_AND_BEGIN);
      c.range(0, 1, 5);
      c.mark(PGPU_F_AND_CHILD_END);
      check(c, 0);
    }
    {
      Case c = base;
      c.name = "missing child end";
      c.mark(PGPU_F_AND_BEGIN);
      c.range(0, 1, 5);
      c.range(1, 1, 5);
      c.mark(PGPU_F_AND_CHILD_END);
      c.mark(PGPU_F_AND_END);
      check(c, 0);
    }
    {
      Case c = base;
      c.name = "wrong child end";
      c.mark(PGPU_F_OR_BEGIN);
      c.range(0, 1, 5);
      c.mark(PGPU_F_AND_CHILD_END);
      c.mark(PGPU_F_OR_END);
      check(c, 0);
    }
    for (int col : {-1, 2}) {
      Case c = base;
      c.name = "column out of range";
      c.range(col, 1, 5);
      check(c, 0);
    }
    {
      Case c = base;
      c.name = "unknown op";
      c.mark(99);
      check(c, 0);
    }
    {
      Case c = base;
      c.name = "trailing nodes";
      c.range(0, 1, 5);
      c.range(1, 1, 5);
      check(c, 0);
    }
    {
      Case c = base;
      c.name = "NOT without a child";
      c.mark(PGPU_F_NOT);
      check(c, 0);
    }
    {
      Case c = base;
      c.name = "raw scan of a dictionary column";
      c.range(0, 0, 0, 0, PGPU_F_RAW_SCAN);
      check(c, 0);
    }
    {
      Case c = base;
      c.name = "a lone child end";
      c.mark(PGPU_F_AND_CHILD_END);
      check(c, 0);
    }
  }
}

// ---- random cases -----------------------------------------------------------------------------------------------

struct Gen {
  std::mt19937_64 rng;
  Case c;
  int budget = 40;
  int pick(int n) { return (int)(rng() % (uint64_t)n); }

  void leaf() {
    const int qc = pick((int)c.cols.size());
    const Col& k = c.cols[qc];
    --budget;
    const int neg = pick(5) == 0;
    if (k.kind == PGPU_COL_RAW) {
      c.range(qc, 0, 0, 0, pick(2) ? PGPU_F_RAW_SCAN : PGPU_F_RANGE_INDEX);
      return;
    }
    if (k.kind == PGPU_COL_SORTED && pick(2)) {
      std::vector<int32_t> v;
      const int n = pick(4);
      for (int j = 0; j < n; ++j) {
        const int s = pick(c.num_docs);
        v.push_back(s);
        v.push_back(s + pick(500) - 20);
      }
      c.set(qc, v, neg, PGPU_F_SORTED);
      return;
    }
    if (!k.inv_cards.empty() && pick(3) == 0) {
      std::vector<int32_t> v;
      const int n = pick(5);
      for (int j = 0; j < n; ++j) v.push_back(pick((int)k.inv_cards.size() + 2) - 1);
      c.set(qc, v, neg, PGPU_F_INVERTED);
      return;
    }
    const int what = pick(10);
    if (what == 0) {
      c.mark(pick(2) ? PGPU_F_MATCH_ALL : PGPU_F_EMPTY);
    } else if (what < 5) {
      const int card = std::max(1, k.card);
      const int lo = pick(card) - (pick(8) == 0 ? 3 : 0);
      const int64_t hi = pick(4) == 0 ? (int64_t)lo + pick(3) : (int64_t)lo + pick(card) + (pick(8) == 0 ? card : 0);
      c.range(qc, lo, (int)std::min<int64_t>(hi, INT32_MAX), neg, pick(6) == 0 ? PGPU_F_RANGE_INDEX : PGPU_F_SCAN);
    } else {
      const int card = std::max(1, k.card);
      const int n = pick(3) == 0 ? pick(70) : pick(10);
      std::vector<int32_t> v;
      for (int j = 0; j < n; ++j) v.push_back(pick(20) == 0 ? card + pick(3) - 1 : pick(card));
      if (pick(2)) std::sort(v.begin(), v.end());
      c.set(qc, v, neg);
    }
  }

  void tree(int depth) {
    const int what = depth >= 6 || budget < 8 ? 9 : pick(10);
    if (what < 3) {
      const bool is_and = pick(2) != 0;
      c.mark(is_and ? PGPU_F_AND_BEGIN : PGPU_F_OR_BEGIN);
      budget -= 2;
      const int n = 1 + pick(4);
      for (int j = 0; j < n && budget > 3; ++j) {
        tree(depth + 1);
        c.mark(is_and ? PGPU_F_AND_CHILD_END : PGPU_F_OR_CHILD_END);
        --budget;
      }
      c.mark(is_and ? PGPU_F_AND_END : PGPU_F_OR_END);
    } else if (what == 3) {
      c.mark(PGPU_F_NOT);
      --budget;
      tree(depth + 1);
    } else {
      leaf();
    }
  }

  void make(uint64_t seed) {
    rng.seed(seed);
    c = Case();
    c.name = "random seed " + std::to_string(seed);
    budget = 40;
    c.num_docs = 1 + pick(100000);
    const int ncols = 2 + pick(5);
    for (int i = 0; i < ncols; ++i) {
      const int kr = pick(12);
      const int kind = kr < 8 ? PGPU_COL_FIXED_BIT : kr < 9 ? PGPU_COL_SORTED : kr < 10 ? PGPU_COL_RAW : kr < 11 ? PGPU_COL_MV : PGPU_COL_NONE;
      const int bits = 1 + pick(32);
      const int64_t top = 1ll << std::min(bits, 30);
      const int card = pick(3) == 0 ? 1 + pick(64) : 1 + (int)(rng() % (uint64_t)top);
      c.col(kind, bits, card, pick(4) != 0);
      if (pick(3) == 0) {
        const int n = std::min(card, 50);
        for (int j = 0; j < n; ++j) c.cols.back().inv_cards.push_back((uint32_t)pick(c.num_docs));
      }
    }
    // mostly a top-level AND, as the planner's interesting programs are
    if (pick(10) < 7) {
      c.mark(PGPU_F_AND_BEGIN);
      budget -= 2;
      const int n = 1 + pick(10);
      for (int j = 0; j < n && budget > 3; ++j) {
        tree(1);
        c.mark(PGPU_F_AND_CHILD_END);
        --budget;
      }
      c.mark(PGPU_F_AND_END);
    } else {
      tree(0);
    }
    // now and then a damaged program
    if (pick(12) == 0 && !c.nodes.empty()) {
      const int at = pick((int)c.nodes.size());
      switch (pick(3)) {
        case 0: c.nodes.erase(c.nodes.begin() + at); break;
        case 1: {  // (never another leaf kind: a leaf's ids are laid out for its own op)
          static const int ops[] = {PGPU_F_MATCH_ALL, PGPU_F_EMPTY, PGPU_F_AND_BEGIN, PGPU_F_AND_CHILD_END,
                                    PGPU_F_AND_END, PGPU_F_OR_BEGIN, PGPU_F_OR_CHILD_END, PGPU_F_OR_END, PGPU_F_NOT,
                                    14, 99, -1};
          c.nodes[at].op = ops[pick(12)];
          break;
        }
        default: c.nodes.resize(at); break;
      }
    }
  }
};

// a damaged program may name a column out of range in a leaf the old lead_choice / scan_runs never reach, but
// every read of a column goes through the same checks in both: nothing to filter here
void random_cases(uint64_t seed, int count) {
  Gen g;
  for (int i = 0; i < count; ++i) {
    g.make(seed + (uint64_t)i);
    if (!check(g.c)) {
      fprintf(stderr, "failing seed: %llu\n", (unsigned long long)(seed + (uint64_t)i));
      return;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "directed")) {
    directed();
  } else if (argc >= 4 && !strcmp(argv[1], "random")) {
    random_cases(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
  } else {
    fprintf(stderr, "usage: segplan_fuzz directed | random SEED COUNT\n");
    return 2;
  }
  if (failures) {
    fprintf(stderr, "%d mismatches\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
