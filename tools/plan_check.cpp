// The invariants the executors rely on, checked over every shape and mode of the launch planner (csrc/bgp_plan.h alone: plain C++).
//
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/plan_check.cpp -o /tmp/plan_check
//   /tmp/plan_check                                         (about 45 minutes), or in 16 processes (6 minutes):
//   for i in $(seq 0 15); do /tmp/plan_check $i 16 & done; wait
//
// Sweep: 1 .. 80 block columns (n up to 10240), nb = 1 .. 256, ncu in {32, 64, 256}, and EVERY combination of: both warp settings,
// matrices built / given, timing, persist, panel_fused, launch-free permitted or not, four settings of panels, four of the streams;
// the three live switches, d and the kernel family in full on the path that reads them (see main).
#include "../bayes-skopt_amd/csrc/bgp_plan.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

static long long g_plans = 0, g_failures = 0;
#define CHECK(cond)                                                                                                        \
  do {                                                                                                                     \
    if (!(cond)) {                                                                                                         \
      if (g_failures++ < 20)                                                                                               \
        fprintf(stderr, "FAILED %s: n=%d nb=%d ncu=%d warped=%d given=%d timing=%d persist=%d fused=%d panels=%d/%d "     \
                        "streams=%d/%d gen=%d pair=%d psgen=%d permitted=%d\n", #cond, s.n, s.nb, s.ncu, s.warped, s.given,   \
                s.timing, s.persist, s.panel_fused, s.panels, s.panels_auto, s.nstreams, s.streams_auto, s.syrk_gen,        \
                s.ps_pair, s.ps_gen, s.ps_permitted);                                                                        \
    }                                                                                                                      \
  } while (0)

static void check(const BgpLmlShape& s) {
  const BgpLmlPlan p = bgp_plan_lml(s);
  g_plans++;
  CHECK(p.path == BGP_PATH_SMALL || p.path == BGP_PATH_LAUNCH_FREE || p.path == BGP_PATH_LAUNCHES);
  CHECK((p.path == BGP_PATH_SMALL) == (s.nblk == 1 && !s.warped && !s.given));
  // groups cover [0, nb) exactly, every group within the streams the context has
  CHECK(p.share >= 1 && p.share <= 8 && p.ngroups >= 1 && p.ngroups <= p.share && p.gsz >= 1);
  CHECK(p.share == 1 || p.gsz % 8 == 0);
  int covered = 0;
  for (int g = 0; g < p.ngroups; g++) {
    CHECK(p.group_nb(g) >= 1 && p.group_nb(g) <= p.gsz);
    covered += p.group_nb(g);
  }
  CHECK(covered == s.nb);
  CHECK(p.P >= 1);
  if (p.path == BGP_PATH_LAUNCH_FREE) {
    CHECK(bgp_persist_fits(s.nblk, s.ncu, s.nb));  // launch-free is chosen only when it fits ...
    CHECK(s.ps_permitted && !s.timing && s.persist != 0);  // ... and is wanted
    CHECK(p.nchain == (p.pair ? 2 * p.Bpad : s.nb) && p.Bpad >= s.nb && p.Bpad % 8 == 0);
    CHECK(p.tile_wgs >= 0 && p.nchain + p.tile_wgs <= s.ncu);
    CHECK(p.tile_wgs <= p.total);
    CHECK(p.ncrit >= 0);
    if (p.total > 0) CHECK(p.tile_wgs >= 1 && p.ncrit <= p.tile_wgs - 1);
    CHECK(p.total == bgp_ps_total_tasks(s.nb, s.nblk, p.psplit, p.ps_gen));
    CHECK(p.psplit == (p.pair ? 4 : 1) && p.dsplit == (p.pair ? 3 : 1));
    if (p.ps_gen) CHECK(!p.pair && p.ncrit == 0 && !s.warped && !s.given && !p.gram_front);
    if (s.warped) CHECK(p.gram_front);
    if (s.given) CHECK(!p.gram_front && !p.ps_gen);
  }
  const BgpLmlLaunches n = bgp_plan_launches(p);
  if (p.path != BGP_PATH_LAUNCHES) {
    CHECK(n.trsm == 0 && n.syrk == 0 && n.fused == 0 && n.generating == 0);
    for (int g = 0; g < p.ngroups; g++) CHECK(p.gen(g) == 0);
    return;
  }
  // the launch schedule: every block column is factorised once, fused or not; every column with a solve is solved once
  long long potrf = 0, solves = 0, fused = 0;
  for (int g = 0; g < p.ngroups; g++) {
    if (s.given || !s.syrk_gen || s.nblk < 2) CHECK(p.gen(g) == 0);
    int next = 0, done_to = 0;  // next block column to factorise; block columns < done_to carry every panel < their index
    bgp_lml_schedule(p, g, [&](const BgpStep& st) {
      const int nrb = s.nblk - st.k - 1;
      switch (st.kind) {
        case BGP_STEP_PANEL:
          CHECK(st.k == next && nrb >= 1);  // a fused column has a solve
          CHECK(st.S >= 1 && st.S <= (nrb > 1 ? nrb : 1));
          CHECK(st.S == p.fused_wgs(g, st.k));
          CHECK((long long)st.S * (8 * ((p.group_nb(g) + 7) / 8)) <= (s.ncu > 8 * ((p.group_nb(g) + 7) / 8) ? s.ncu : 8 * ((p.group_nb(g) + 7) / 8)));
          CHECK(s.panel_fused != 0);
          next++, fused++, solves++;
          break;
        case BGP_STEP_POTRF:
          CHECK(st.k == next && p.fused_wgs(g, st.k) == 0);
          next++, potrf++;
          break;
        case BGP_STEP_TRSM:
          CHECK(st.k == next - 1 && nrb >= 1);
          solves++;
          break;
        case BGP_STEP_COLUMN:
          CHECK(st.j == next && st.j < s.nblk && st.K == 128 * (st.j - st.k) && st.K >= 128 && st.K <= 128 * (p.P - 1));
          CHECK(!st.gen || (p.gen(g) && st.k == 0));
          break;
        case BGP_STEP_UPDATE:
          CHECK(st.j == next && st.j < s.nblk && st.K == 128 * (st.j - st.k) && st.K <= 128 * p.P && st.k == done_to);
          CHECK(!st.gen || (p.gen(g) && st.k == 0));
          done_to = st.j;
          break;
        default:
          CHECK(false);
      }
    });
    CHECK(next == s.nblk);
  }
  CHECK(potrf + fused == (long long)p.ngroups * s.nblk && solves == (long long)p.ngroups * (s.nblk - 1));
  CHECK(n.potrf == potrf && n.fused == fused && n.trsm == solves && n.columns <= n.syrk);
  CHECK(n.kbuild == (s.given ? 0 : p.ngroups));
}

// Every combination of the modes -- warped, given, timing, persist, panel_fused, launch-free permitted, panels, streams -- meets
// every (block columns, matrices, CUs).  The path depends on none of the live switches, d or the kernel family, and each of
// those is read on one path only: BGP_SYRK_GEN and d by the launch schedule (BgpLmlPlan::gen), BGP_PS_PAIR, BGP_PS_GEN and the
// family by the launch-free layout; the n <= 128 launch reads none.  So they are crossed in full ON the path that reads them
// (checked below: the path is the same for all of them), not on the others, where the plan cannot differ.
// argv: `part parts` runs the block-column counts with nblk % parts == part (the sweep in parallel processes).
int main(int argc, char** argv) {
  const int part = argc > 2 ? atoi(argv[1]) : 0, parts = argc > 2 ? atoi(argv[2]) : 1;
  static const int ncus[] = {32, 64, 256};
  static const int panels[][2] = {{2, 1}, {1, 0}, {3, 0}, {64, 0}};   // {panels, panels_auto}
  static const int streams[][2] = {{1, 1}, {2, 1}, {2, 0}, {8, 0}};  // {nstreams, streams_auto}
  for (int blk = 1; blk <= 80; blk++) {
    if (blk % parts != part) continue;
    for (int nb = 1; nb <= 256; nb++)
      for (int ncu : ncus)
        for (int mode = 0; mode < 2 * 2 * 2 * 3 * 3 * 2 * 4 * 4; mode++) {
          BgpLmlShape s{};
          int m = mode;
          // (n enters the plan through its block columns alone: the last size of each count; 128 blk - 127 gives the same plans)
          s.n = 128 * blk, s.nblk = blk, s.ncu = ncu, s.nb = nb;
          s.warped = m % 2, m /= 2;
          s.given = m % 2, m /= 2;
          s.timing = m % 2, m /= 2;
          s.persist = m % 3 - 1, m /= 3;
          s.panel_fused = m % 3 - 1, m /= 3;
          s.ps_permitted = m % 2, m /= 2;
          s.panels = panels[m % 4][0], s.panels_auto = panels[m % 4][1], m /= 4;
          s.nstreams = streams[m % 4][0], s.streams_auto = streams[m % 4][1], m /= 4;
          if (s.warped && s.given) continue;
          s.d = 4, s.stationary = BGP_PLAN_MATERN52, s.form = BGP_PLAN_FORM_PRODUCT, s.syrk_gen = 1, s.ps_pair = s.ps_gen = -1;
          const int path = bgp_plan_lml(s).path;
          if (path == BGP_PATH_SMALL) {
            check(s);
          } else if (path == BGP_PATH_LAUNCHES) {
            for (int v = 0; v < 4; v++) {
              s.syrk_gen = v % 2, s.d = v / 2 ? 20 : 4;
              CHECK(bgp_plan_lml(s).path == path);
              check(s);
            }
          } else {
            for (int v = 0; v < 18; v++) {
              s.ps_pair = v % 3 - 1, s.ps_gen = v / 3 % 3 - 1, s.stationary = v / 9 ? 0 : BGP_PLAN_MATERN52;
              CHECK(bgp_plan_lml(s).path == path);
              check(s);
            }
          }
        }
  }
  printf("plan_check: %lld plans, %lld failures\n", g_plans, g_failures);
  return g_failures ? 1 : 0;
}
