// plan_probe — prints what csrc/plan.h decides for a shape, on any machine: no GPU, no HIP.
//   c++ -std=c++17 -O1 -o plan_probe tests/helpers/plan_probe.cpp && echo "10000 64 8192 0 0x6020" | ./plan_probe
// stdin, one shape per line:  M D n dtype flags [key=value ...] [set:key=value ...]
//   key=value      an option given to rmhmc_create_opts
//   set:key=value  an option given to rmhmc_set_option afterwards (checked, then applied)
// stdout, one JSON object per line: "check" (plan_check), "option_error" (the first option refused, or null) and, when both pass,
// "plan" (every field of Plan), "i8" (the launch geometry of the int8 assembly for the plan's own tile shape and batch, with the k
// pieces of one assembly) and "amh" (amh_shape).
#include "../../riemannhamiltonianmontecarlo_amd/csrc/plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    long long M, n;
    int D, dtype;
    std::string fl;
    if (!(in >> M >> D >> n >> dtype >> fl)) continue;
    const uint32_t flags = (uint32_t)std::strtoul(fl.c_str(), nullptr, 0);
    Options opt{};
    std::string bad_key, bad_why, bad_at;
    for (std::string tok; bad_key.empty() && in >> tok;) {
      const bool set = tok.rfind("set:", 0) == 0;
      if (set) tok = tok.substr(4);
      const size_t eq = tok.find('=');
      const std::string key = tok.substr(0, eq);
      const int64_t value = eq == std::string::npos ? 0 : std::strtoll(tok.c_str() + eq + 1, nullptr, 0);
      const OptionDesc* d = find_option(key.c_str());
      const OptionError e = check_option(d, value, !set);
      if (e == OPT_OK) { opt.*(d->slot) = value; continue; }
      bad_key = key; bad_at = set ? "set" : "create";
      bad_why = e == OPT_UNKNOWN ? "unknown" : e == OPT_CREATE_ONLY ? "create_only" : "range";
    }
    const PlanCheck chk = plan_check(M, D, n, dtype, flags);
    std::printf("{\"check\": {\"code\": %d, \"msg\": \"%s\"}, \"option_error\": ", chk.code, chk.msg);
    if (bad_key.empty()) std::printf("null");
    else std::printf("{\"key\": \"%s\", \"why\": \"%s\", \"at\": \"%s\"}", bad_key.c_str(), bad_why.c_str(), bad_at.c_str());
    if (chk.code != RMHMC_OK || !bad_key.empty()) { std::printf("}\n"); continue; }
    const Plan p = make_plan(M, D, n, flags, opt);
    std::printf(", \"plan\": {\"M\": %lld, \"D\": %d, \"n\": %lld, \"NB\": %d, \"DP\": %d, \"Mp\": %d, \"nblk\": %d, \"big\": %d, \"nbk\": %d, \"npairs\": %d, "
                "\"nsplit\": %d, \"fsplit\": %d, \"gpart_planes\": %d, \"hpart_at_create\": %d, ",
                (long long)p.M, p.D, (long long)p.n, p.NB, p.DP, p.Mp, p.nblk, (int)p.big, p.nbk, p.npairs, p.nsplit, p.fsplit, p.gpart_planes,
                (int)p.hpart_at_create);
    std::printf("\"i8_requested\": %d, \"i8S\": %d, \"i8_chunk\": %d, \"i8_bn\": %d, \"i8_nks\": %d, \"NP\": %d, \"NPp\": %d, \"i8_nkp\": %d, \"i8_NRp\": %d, "
                "\"nCp\": %d, \"ksplit_a\": %d, \"ksplit_l\": %d, \"tail_acc\": %d, \"tail_always\": %d, \"tail_pieces\": %d, \"tail_blocks\": %d, \"gbase\": %d, \"i8_lev_full\": %d, ",
                (int)p.i8_requested, p.i8S, p.i8_chunk, p.i8_bn, p.i8_nks, p.NP, p.NPp, p.i8_nkp, p.i8_NRp, p.nCp, p.ksplit_a, p.ksplit_l, (int)p.tail_acc,
                (int)p.tail_always, p.tail_pieces, p.tail_blocks, (int)p.gbase, (int)p.i8_lev_full);
    std::printf("\"fused\": %d, \"fused_lds\": %zu, \"medium\": %d, \"medium_lds\": %zu, \"hmc_traj\": %d}", (int)p.fused, p.fused_lds, (int)p.medium,
                p.medium_lds, (int)p.hmc_traj);
    if (p.i8_requested) {
      const int WN = i8_tile_wn(p.i8S), TN = i8_tile_tn(p.i8S);
      const I8Geometry g = i8_geometry(p, p.nCp, WN, TN, WN == 4);
      std::printf(", \"i8\": {\"WN\": %d, \"TN\": %d, \"nCB\": %d, \"nPB\": %d, \"nPBfull\": %d, \"tail\": %d, \"npb\": %d, \"nblk_main\": %u, \"pb32_0\": %d, "
                  "\"ntail\": %d, \"k_pieces\": [",
                  WN, TN, g.nCB, g.nPB, g.nPBfull, (int)g.tail, g.npb, g.nblk_main, g.pb32_0, g.ntail);
      for (int ks0 = 0; ks0 < p.i8_nks; ks0 += p.i8_chunk) {  // (the loop of launch_assemble_i8_t)
        const int nk = std::min(p.i8_chunk, p.i8_nks - ks0);
        std::printf("%s{\"ks0\": %d, \"nk\": %d, \"tail_pieces\": %d}", ks0 ? ", " : "", ks0, nk, i8_tail_pieces(p, g, nk));
      }
      std::printf("]}");
    }
    const AmhShape a = amh_shape(M, n);
    std::printf(", \"amh\": {\"nt\": %d, \"rows\": %d}}\n", a.nt, a.rows);
  }
  return 0;
}
