// CPU driver for the gather choice of the MFMA conv's host planner
// (ops/csrc/conv_plan.h, gather_eligible), built with the host compiler under
// the sanitizers by tests/test_conv_gather_plan_cpu.py. Reads one command per
// line on stdin, prints one JSON object per command. Pointers are plain
// integers: the planner compares them, it never dereferences one.
//
//   plan <geom x15> x w x2 cin2 push   plan_conv; push=1 appends the plan to
//                                      the group list
//   group                              assemble_group over the pushed plans:
//                                      the gather and cfg of every grid slot
//   clear                              empty the group list
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "conv_plan.h"

namespace {

template <class T>
T* ptr(unsigned long long v) { return reinterpret_cast<T*>((uintptr_t)v); }

void plan(std::istringstream& in, std::vector<ibp::ConvPlan>& plans) {
  ibp::ConvProblem prob;
  ibp::ConvParams& q = prob.p;
  int* geom[15] = {&q.N, &q.H, &q.W, &q.Cin, &q.Cout, &q.KH, &q.KW,
                   &q.stride, &q.pad_h, &q.pad_w, &q.dil_h, &q.dil_w,
                   &q.Ho, &q.Wo, &q.zs};
  for (int* g : geom) in >> *g;
  unsigned long long x, w, x2;
  int push;
  in >> x >> w >> x2 >> q.Cin2 >> push;
  if (!in) throw std::invalid_argument("plan: malformed command");
  q.x = ptr<const unsigned short>(x);
  q.w = ptr<const unsigned short>(w);
  q.x2 = ptr<const unsigned short>(x2);
  q.y = ptr<unsigned short>(1ull << 40);
  const ibp::ConvPlan pl = ibp::plan_conv(prob);
  if (push) plans.push_back(pl);
  std::printf("{\"gather\": %d, \"m32\": %d, \"BM\": %d, \"BN\": %d, "
              "\"splitk\": %d, \"deep\": %d, \"K\": %d, \"M\": %lld}\n",
              pl.p.gather, pl.p.m32, pl.t.BM, pl.t.BN, pl.p.splitk,
              (int)pl.t.deep, pl.p.K, pl.p.M);
}

void group(std::vector<ibp::ConvPlan>& plans) {
  const ibp::GroupPlan gp =
      ibp::assemble_group(plans, 0, plans.size(), ptr<float>(1ull << 41));
  std::printf("{\"n\": %d, \"order\": [", gp.g.n);
  for (int i = 0; i < gp.g.n; ++i)
    std::printf("%s%d", i ? ", " : "", gp.order[i]);
  std::printf("], \"gather\": [");
  for (int i = 0; i < ibp::kMaxGroup; ++i)
    std::printf("%s%d", i ? ", " : "", gp.g.p[i].gather);
  std::printf("], \"cfg\": [");
  for (int i = 0; i < ibp::kMaxGroup; ++i)
    std::printf("%s%d", i ? ", " : "", gp.g.cfg[i]);
  std::printf("]}\n");
}

}  // namespace

int main() {
  std::vector<ibp::ConvPlan> plans;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    try {
      if (cmd == "plan") {
        plan(in, plans);
      } else if (cmd == "group") {
        group(plans);
      } else if (cmd == "clear") {
        plans.clear();
        std::printf("{}\n");
      } else {
        throw std::invalid_argument("unknown command " + cmd);
      }
    } catch (const std::invalid_argument& e) {
      std::printf("{\"error\": \"%s\"}\n", e.what());
    }
  }
  return 0;
}
