// CPU driver for the two-source guards of the MFMA conv's host planner
// (ops/csrc/conv_plan.h), built with the host compiler under the sanitizers by
// tests/test_cat_conv_cpu.py. One command per line on stdin, one JSON object
// per command on stdout. Pointers are plain integers, never dereferenced.
//
//   conv <geom x15> x x2 Cin2 up tile push
//                                 plan_conv of a conv with second source x2
//                                 (0 = none) of Cin2 channels; tile=1 hands it
//                                 a tile chosen elsewhere; push=1 appends the
//                                 plan to the group list
//   group first last ws_base      assemble_group over the pushed plans
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

void conv(std::istringstream& in, std::vector<ibp::ConvPlan>& plans) {
  ibp::ConvProblem prob;
  ibp::ConvParams& q = prob.p;
  int* geom[15] = {&q.N, &q.H, &q.W, &q.Cin, &q.Cout, &q.KH, &q.KW,
                   &q.stride, &q.pad_h, &q.pad_w, &q.dil_h, &q.dil_w,
                   &q.Ho, &q.Wo, &q.zs};
  for (int* g : geom) in >> *g;
  unsigned long long x, x2;
  int tile, push;
  in >> x >> x2 >> q.Cin2 >> q.up >> tile >> push;
  if (!in) throw std::invalid_argument("conv: malformed command");
  q.x = ptr<const unsigned short>(x);
  q.x2 = ptr<const unsigned short>(x2);
  q.w = ptr<const unsigned short>(1ull << 30);
  q.y = ptr<unsigned short>(1ull << 31);
  if (tile)
    prob.tile = ibp::plan_tile((long long)q.N * q.Ho * q.Wo, q.Cout,
                               q.KH * q.KW * q.Cin);
  const ibp::ConvPlan plan = ibp::plan_conv(prob);
  if (push) plans.push_back(plan);
  const ibp::ConvParams& p = plan.p;
  std::printf("{\"BM\": %d, \"BN\": %d, \"splitk\": %d, \"deep\": %d, "
              "\"nk_block\": %d, \"nblocks\": %d, \"ws_elems\": %lld, "
              "\"M\": %lld, \"K\": %d, \"Cin\": %d, \"Cin2\": %d, "
              "\"x2\": %llu, \"vec_epi\": %d}\n",
              plan.t.BM, plan.t.BN, p.splitk, (int)plan.t.deep,
              plan.t.nk_block, plan.nblocks, plan.ws_elems, p.M, p.K, p.Cin,
              p.Cin2, (unsigned long long)(uintptr_t)p.x2, p.vec_epi);
}

void group(std::istringstream& in, std::vector<ibp::ConvPlan>& plans) {
  size_t first, last;
  unsigned long long ws_base;
  in >> first >> last >> ws_base;
  if (!in) throw std::invalid_argument("group: malformed command");
  const ibp::GroupPlan gp =
      ibp::assemble_group(plans, first, last, ptr<float>(ws_base));
  std::printf("{\"n\": %d, \"blocks\": %d}\n", gp.g.n, gp.blocks);
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
      if (cmd == "conv") conv(in, plans);
      else if (cmd == "group") group(in, plans);
      else throw std::invalid_argument("unknown command " + cmd);
    } catch (const std::invalid_argument& e) {
      std::printf("{\"error\": \"%s\"}\n", e.what());
    }
  }
  return 0;
}
