// Host-only harness for the launch choice (fruits_amd/csrc/launch_choice.h), built by
// tests/test_host.py::test_launch_choice_table with plan.cpp - plainly, and with
// -fsanitize=address,undefined.  Reads from stdin: the number of plans, every plan as
// plan_sanitize.cpp reads one (W weighting flags; per word L Dw depth, L*Dw exponents, L
// alphas); then the number of cases and per case
//   plan N T groups fused total_inc carry_per_node vec_ok resident aot1 aot2 aot3 jit_mask
//   tail_groups mixed_R | knobs: groups persist packed lean wt tail static_cache_x100
//   static_min_T FRUITS_HIP_STATIC
// and prints every field of the WalkChoice, and how often the mixed instance was asked; then, on a
// line of its own, the launch as fr_plan_info reports it (pack_last_launch) and what reads back from
// that word (unpack_last_launch).  A field that does not read back as it went in ends the run.
#include <cstdio>
#include <string>
#include <vector>

#include "../../fruits_amd/csrc/launch_choice.h"

int main() {
  int n_plans = 0, n_cases = 0;
  if (scanf("%d", &n_plans) != 1) return 2;
  std::vector<fr::Plan *> plans;
  for (int c = 0; c < n_plans; ++c) {
    int W, weighting, flags;
    if (scanf("%d %d %d", &W, &weighting, &flags) != 3) return 2;
    std::vector<int32_t> exps, L(W), Dw(W), depth(W);
    std::vector<float> alpha;
    for (int i = 0; i < W; ++i) {
      if (scanf("%d %d %d", &L[i], &Dw[i], &depth[i]) != 3) return 2;
      for (int j = 0; j < L[i] * Dw[i]; ++j) {
        int e;
        if (scanf("%d", &e) != 1) return 2;
        exps.push_back(e);
      }
      for (int j = 0; j < L[i]; ++j) {
        float a;
        if (scanf("%f", &a) != 1) return 2;
        alpha.push_back(a);
      }
    }
    std::string err;
    fr::Plan *p = fr::build_plan(W, exps.data(), L.data(), Dw.data(), weighting ? alpha.data() : nullptr,
                                 depth.data(), weighting, flags, err);
    if (!p) {
      printf("plan %d: rejected: %s\n", c, err.c_str());
      return 3;
    }
    printf("plan %d: K=%d nodes=%zu levels=%d units=%d rows=%d\n", c, p->K, p->nodes.size(), p->levels,
           p->units(), p->rows_staged());
    plans.push_back(p);
  }
  if (scanf("%d", &n_cases) != 1) return 2;
  for (int c = 0; c < n_cases; ++c) {
    int plan, fused, total_inc, vec_ok, jit_mask;
    long long N, T, resident, mixed_R;
    fr::WalkFacts f;
    fr::WalkKnobs k;
    if (scanf("%d %lld %lld %d %d %d %d %d %lld %d %d %d %d %d %lld", &plan, &N, &T, &f.groups, &fused,
              &total_inc, &f.carry_per_node, &vec_ok, &resident, &f.aot[1], &f.aot[2], &f.aot[3],
              &jit_mask, &f.tail_groups, &mixed_R) != 15)
      return 2;
    if (scanf("%d %d %d %d %d %d %d %d %d", &k.groups, &k.persist, &k.packed, &k.lean, &k.wt, &k.tail,
              &k.static_cache_x100, &k.static_min_T, &k.hip_static) != 9)
      return 2;
    if (plan < 0 || plan >= (int)plans.size()) return 2;
    fr::Plan &p = *plans[plan];
    f.N = N;
    f.T = T;
    f.fused = fused != 0;
    f.total_inc = total_inc != 0;
    f.vec_ok = vec_ok != 0;
    f.resident = resident;
    for (int g = 1; g <= 3; ++g) f.jit[g] = (jit_mask >> g & 1) != 0;
    int asked = 0;
    f.mixed_resident = [&] {
      ++asked;
      return (int64_t)mixed_R;
    };
    f.largest_group = [&p](int G) { return fr::largest_group(fr::grouped(p, G)); };
    const fr::WalkChoice ch = fr::choose_walk_launch(p, f, k);
    printf("case %d: packed=%d G=%d static=%d wt=%d pad=%d cache=%d lean=%d persistent=%d nt=%d "
           "slots=%d per_node=%d in_lds=%d tail=%lld whole=%d xcd=%d mixed_asked=%d\n",
           c, ch.packed ? 1 : 0, ch.G, ch.static_prog, ch.wt, ch.lds_pad, ch.cache_sized ? 1 : 0, ch.lean,
           ch.persistent, ch.nt_input, ch.carry_slots, ch.carry_per_node, ch.carry_in_lds,
           (long long)ch.tail_series, ch.n_whole, ch.xcd_map, asked);
    fr::LastLaunch rec;
    rec.choice = ch;
    rec.family = fr::walk_family(ch, f.fused);
    rec.resident = f.resident;
    rec.mixed_resident = asked ? mixed_R : 0;
    const int64_t word = fr::pack_last_launch(rec);
    const fr::LastLaunch back = fr::unpack_last_launch(word);
    printf("launch %d: word=%lld family=%d G=%d persistent=%d xcd=%d nt=%d wt=%d pad=%d in_lds=%d "
           "resident=%lld mixed=%lld\n",
           c, (long long)word, back.family, back.choice.G, back.choice.persistent, back.choice.xcd_map,
           back.choice.nt_input, back.choice.wt, back.choice.lds_pad, back.choice.carry_in_lds,
           (long long)back.resident, (long long)back.mixed_resident);
    auto sat = [](int64_t v, int bits) { return v < 0 ? 0 : (v >> bits ? (int64_t(1) << bits) - 1 : v); };
    if (word <= 0 || back.family != rec.family || back.choice.G != sat(ch.G, 8) ||
        back.choice.persistent != sat(ch.persistent, 4) || back.choice.xcd_map != (ch.xcd_map != 0) ||
        back.choice.nt_input != (ch.nt_input != 0) || back.choice.wt != (ch.wt != 0) ||
        back.choice.lds_pad != (ch.lds_pad != 0) || back.choice.carry_in_lds != (ch.carry_in_lds != 0) ||
        back.resident != sat(rec.resident, 20) || back.mixed_resident != sat(rec.mixed_resident, 20)) {
      printf("launch %d: the word does not read back\n", c);
      return 4;
    }
  }
  // fields beyond their width read as the width's largest value and disturb no neighbour
  {
    fr::LastLaunch big;
    big.family = fr::kWalkFusedPieces;
    big.choice.G = 1000;
    big.choice.persistent = 99;
    big.resident = int64_t(1) << 40;
    big.mixed_resident = -5;
    const fr::LastLaunch back = fr::unpack_last_launch(fr::pack_last_launch(big));
    if (back.family != fr::kWalkFusedPieces || back.choice.G != 255 || back.choice.persistent != 15 ||
        back.resident != 0xfffff || back.mixed_resident != 0 || back.choice.xcd_map || back.choice.wt ||
        back.choice.nt_input || back.choice.lds_pad || back.choice.carry_in_lds != 0 ||
        fr::pack_last_launch(fr::LastLaunch{}) != 0) {
      printf("saturation: the word does not read back\n");
      return 4;
    }
    printf("saturation: ok\n");
  }
  for (fr::Plan *p : plans) delete p;
  return 0;
}
