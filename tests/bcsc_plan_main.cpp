// Prints what plan_bcsc (libxsmm_amd/csrc/bcsc_plan.hpp) decides, without a GPU: one BcscArgs per input line as integers
//   a bvals c  M N K m_blocks bk bn  a_type b_type c_type vnni_a beta0  table stream_hint nt_a table_ready kmask0 nnzb
// (a, bvals, c: the addresses; table: 0 or not), one line of key=value fields per input line, "name=(empty)" where launch_bcsc launches nothing.
// Built by tests/test_bcsc_plan_cpu.py with g++ alone; stand-alone so that it can also be built with -fsanitize=address,undefined.
#include <cstdio>
#include "../libxsmm_amd/csrc/bcsc_plan.hpp"

int main() {
  char line[1024];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long pa, pb, pc, table, kmask0;
    xamd::BcscArgs a{};
    const int got = std::sscanf(line, "%llu %llu %llu %d %d %d %d %d %d %d %d %d %d %d %llu %d %d %d %llu %d", &pa, &pb, &pc, &a.M, &a.N, &a.K, &a.m_blocks, &a.bk, &a.bn,
                                &a.a_type, &a.b_type, &a.c_type, &a.vnni_a, &a.beta0, &table, &a.stream_hint, &a.nt_a, &a.table_ready, &kmask0, &a.nnzb);
    if (got != 20) { std::fprintf(stderr, "expected 20 integers, read %d: %s", got, line); return 2; }
    a.a = (const char*)(size_t)pa; a.bvals = (const char*)(size_t)pb; a.c = (char*)(size_t)pc; a.table = (void*)(size_t)table; a.kmask0 = kmask0;
    if (xamd::bcsc_empty(a)) { std::puts("name=(empty)"); continue; }
    const xamd::BcscPlan p = xamd::plan_bcsc(a);
    std::printf("name=%s family=%d form=%d bn_sel=%d nt_a=%d early=%d b_lds=%d ua=%d depth=%d tiles_i=%u tiles_n=%u total=%lld mbg=%lld waves=%lld nkb=%d invert=%d three=%d\n",
                p.name, (int)p.family, (int)p.form, p.bn_sel, p.nt_a, p.early, p.b_lds, p.ua, p.depth, p.tiles_i, p.tiles_n, p.total, p.mbg, p.waves, p.nkb, (int)p.invert,
                XAMD_BCSC_THREE != 0);
  }
  return 0;
}
