// CPU driver for the MFMA conv's host planner (ops/csrc/conv_plan.h), built
// with the host compiler under the sanitizers by tests/test_conv_plan_cpu.py.
// Reads one command per line on stdin, prints one JSON object per command.
// Pointers are plain integers: the planner compares and offsets them, it
// never dereferences one.
//
//   tile M Cout K                 plan_tile
//   uptile M_low Cout Cin         plan_upfold_tile
//   sweep NT NK                   pick_split over ntiles 1..NT x nk_total 1..NK
//   conv <geom x15> x w y scale shift res post post2 act up py px ws push
//                                 plan_conv; up=1 is one parity of an upfold
//                                 conv and takes plan_upfold_tile's tile;
//                                 push=1 appends the plan to the group list,
//                                 push=0 completes it with workspace `ws`
//   group first last ws_base      assemble_group over the pushed plans
//   clear                         empty the group list
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

unsigned long long num(const void* p) { return (unsigned long long)(uintptr_t)p; }

template <class F>
void list(const char* key, int n, F&& f, const char* end = ", ") {
  std::printf("\"%s\": [", key);
  for (int i = 0; i < n; ++i)
    std::printf("%s%lld", i ? ", " : "", (long long)f(i));
  std::printf("]%s", end);
}

void print_tile(const ibp::TilePlan& t) {
  std::printf("{\"BM\": %d, \"BN\": %d, \"splitk\": %d, \"deep\": %d, "
              "\"n_mtiles\": %d, \"ntiles\": %d, \"nk_block\": %d}\n",
              t.BM, t.BN, t.splitk, (int)t.deep, t.n_mtiles, t.ntiles,
              t.nk_block);
}

void sweep(int NT, int NK) {
  long long cases = 0, bad = 0;
  int first[3] = {0, 0, 0};
  for (int nt = 1; nt <= NT; ++nt)
    for (int nk = 1; nk <= NK; ++nk) {
      const int sk = ibp::pick_split(nt, nk);
      ++cases;
      // every slice s < sk starts inside the K range: no slice without work
      const bool ok = sk >= 1 && sk <= nk &&
                      (long long)(sk - 1) * ((nk + sk - 1) / sk) < nk;
      if (!ok && !bad++) { first[0] = nt; first[1] = nk; first[2] = sk; }
    }
  std::printf("{\"cases\": %lld, \"bad\": %lld, \"first_bad\": [%d, %d, %d]}\n",
              cases, bad, first[0], first[1], first[2]);
}

void conv(std::istringstream& in, std::vector<ibp::ConvPlan>& plans) {
  ibp::ConvProblem prob;
  ibp::ConvParams& q = prob.p;
  int* geom[15] = {&q.N, &q.H, &q.W, &q.Cin, &q.Cout, &q.KH, &q.KW,
                   &q.stride, &q.pad_h, &q.pad_w, &q.dil_h, &q.dil_w,
                   &q.Ho, &q.Wo, &q.zs};
  for (int* g : geom) in >> *g;
  unsigned long long a[8], ws;
  for (auto& v : a) in >> v;
  int push;
  in >> q.act >> q.up >> q.py >> q.px >> ws >> push;
  if (!in) throw std::invalid_argument("conv: malformed command");
  q.x = ptr<const unsigned short>(a[0]);
  q.w = ptr<const unsigned short>(a[1]);
  q.y = ptr<unsigned short>(a[2]);
  q.scale = ptr<const float>(a[3]);
  q.shift = ptr<const float>(a[4]);
  q.res = ptr<const unsigned short>(a[5]);
  q.res_post = ptr<const unsigned short>(a[6]);
  q.res_post2 = ptr<const unsigned short>(a[7]);
  if (q.up)
    prob.tile = ibp::plan_upfold_tile((long long)q.N * q.Ho * q.Wo, q.Cout,
                                      q.Cin);
  ibp::ConvPlan plan = ibp::plan_conv(prob);
  if (push) plans.push_back(plan);
  else if (plan.ws_elems > 0) ibp::set_workspace(plan, ptr<float>(ws));
  const ibp::ConvParams& p = plan.p;
  std::printf("{\"BM\": %d, \"BN\": %d, \"splitk\": %d, \"deep\": %d, "
              "\"vec_epi\": %d, \"pair_epi\": %d, \"vec_combine\": %d, "
              "\"m32\": %d, \"nblocks\": %d, \"nk_block\": %d, "
              "\"ws_elems\": %lld, \"n_mtiles\": %d, \"M\": %lld, \"K\": %d, "
              "\"up\": %d, \"py\": %d, \"px\": %d, \"cfg\": %d, "
              "\"combine_blocks\": %d}\n",
              plan.t.BM, plan.t.BN, p.splitk, (int)plan.t.deep, p.vec_epi,
              p.pair_epi, (int)plan.vec_combine, p.m32, plan.nblocks,
              plan.t.nk_block, plan.ws_elems, p.n_mtiles, p.M, p.K, p.up, p.py,
              p.px, ibp::tile_cfg(plan.t.BM, plan.t.BN, plan.t.deep),
              ibp::combine_blocks(plan));
}

void group(std::istringstream& in, std::vector<ibp::ConvPlan>& plans) {
  size_t first, last;
  unsigned long long ws_base;
  in >> first >> last >> ws_base;
  if (!in) throw std::invalid_argument("group: malformed command");
  // the size is asked for first, as the caller that has to allocate it does
  const long long ws_total = ibp::group_workspace(plans, first, last);
  const ibp::GroupPlan gp =
      ibp::assemble_group(plans, first, last, ptr<float>(ws_base));
  const int n = gp.g.n, K = ibp::kMaxGroup;
  std::printf("{\"n\": %d, \"blocks\": %d, \"cblocks\": %d, \"up\": %d, "
              "\"ws_total\": %lld, ",
              n, gp.blocks, gp.cblocks, (int)gp.up, ws_total);
  list("order", n, [&](int i) { return gp.order[i]; });
  list("ws_off", n, [&](int i) { return gp.ws_off[i]; });
  list("block_end", K, [&](int i) { return gp.g.block_end[i]; });
  list("cfg", K, [&](int i) { return gp.g.cfg[i]; });
  list("y", K, [&](int i) { return num(gp.g.p[i].y); });
  list("ws", K, [&](int i) { return num(gp.g.p[i].ws); });
  list("splitk", K, [&](int i) { return gp.g.p[i].splitk; });
  std::printf("\"cn\": %d, ", gp.cg.n);
  list("c_block_end", K, [&](int i) { return gp.cg.block_end[i]; });
  list("c_y", K, [&](int i) { return num(gp.cg.c[i].y); });
  list("c_ws", K, [&](int i) { return num(gp.cg.c[i].ws); });
  list("c_vec", K, [&](int i) { return gp.cg.c[i].vec; });
  list("c_total", K, [&](int i) { return gp.cg.c[i].total; });
  list("c_up", K, [&](int i) { return gp.cg.c[i].os.up; });
  list("c_splitk", K, [&](int i) { return gp.cg.c[i].splitk; }, "}\n");
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
      if (cmd == "tile") {
        long long M; int Cout, K;
        in >> M >> Cout >> K;
        print_tile(ibp::plan_tile(M, Cout, K));
      } else if (cmd == "uptile") {
        long long M; int Cout, Cin;
        in >> M >> Cout >> Cin;
        print_tile(ibp::plan_upfold_tile(M, Cout, Cin));
      } else if (cmd == "sweep") {
        int NT, NK;
        in >> NT >> NK;
        sweep(NT, NK);
      } else if (cmd == "conv") {
        conv(in, plans);
      } else if (cmd == "group") {
        group(in, plans);
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
