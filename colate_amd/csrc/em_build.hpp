// colate_amd/csrc/em_build.hpp -- which instantiation of the EM kernel (em_kernel_impl.hpp) a launch takes: one table and
// one pure function.  Host code without HIP: em_kernels*.hip launch by it, colate_api.cpp reports it
// (colate_em_kernel_build*), tests/test_em_builds_cpu.py walks it without a device.
//
//   unit      translation unit           how it is built
//   ilp       em_kernels_ilp.hip         max-ilp machine scheduler
//   default   em_kernels.hip             default scheduler
//   big       em_kernels_big.hip         default scheduler; 8 and 16 epochs per lane, general loop only
//
//   kind      template arguments         what it is
//   free      <0, 1, EROWS, false, 2>    latency layout (a wave per role and bin group), two barriers per iteration, no
//                                        register cap: every workgroup has a CU to itself
//   capped    <0, NCH, EROWS, false>     latency layout, three barriers, registers capped for several workgroups on a CU
//   tput      <0, NCH, EROWS, true>      throughput layout: two waves per replicate that walk through the bin groups
//   estep     <1, NCH, 4, false>         one E-step (colate_em_estep)
//
// A build's name is `unit-kind/NCHxEROWS` (NCH: epochs per lane, EROWS: 16-lane rows of epochs the scans span).
#pragma once
#include <cstring>

enum { kEmUnitIlp = 0, kEmUnitDefault = 1, kEmUnitBig = 2 };

struct EmBuild {
  const char* name;
  int mode;  // 0 = EM to convergence, 1 = one E-step
  int unit;
  int nch, erows;
  bool tput;
  int wpe;  // the WPE template argument: 2 = the free build, 0 = waves per SIMD by NCH
};

// every instantiation the three units hold
inline constexpr EmBuild kEmBuilds[] = {
    {"ilp-free/1x1", 0, kEmUnitIlp, 1, 1, false, 2},
    {"ilp-free/1x2", 0, kEmUnitIlp, 1, 2, false, 2},
    {"ilp-free/1x4", 0, kEmUnitIlp, 1, 4, false, 2},
    {"ilp-capped/1x1", 0, kEmUnitIlp, 1, 1, false, 0},
    {"ilp-capped/1x2", 0, kEmUnitIlp, 1, 2, false, 0},
    {"ilp-capped/1x4", 0, kEmUnitIlp, 1, 4, false, 0},
    {"ilp-capped/2x4", 0, kEmUnitIlp, 2, 4, false, 0},
    {"default-capped/1x1", 0, kEmUnitDefault, 1, 1, false, 0},
    {"default-capped/1x2", 0, kEmUnitDefault, 1, 2, false, 0},
    {"default-capped/1x4", 0, kEmUnitDefault, 1, 4, false, 0},
    {"default-capped/2x4", 0, kEmUnitDefault, 2, 4, false, 0},
    {"default-tput/1x1", 0, kEmUnitDefault, 1, 1, true, 0},
    {"default-tput/1x2", 0, kEmUnitDefault, 1, 2, true, 0},
    {"default-tput/1x4", 0, kEmUnitDefault, 1, 4, true, 0},
    {"default-tput/2x4", 0, kEmUnitDefault, 2, 4, true, 0},
    {"default-tput/4x4", 0, kEmUnitDefault, 4, 4, true, 0},
    {"big-tput/8x4", 0, kEmUnitBig, 8, 4, true, 0},
    {"big-tput/16x4", 0, kEmUnitBig, 16, 4, true, 0},
    {"default-estep/1x4", 1, kEmUnitDefault, 1, 4, false, 0},
    {"default-estep/2x4", 1, kEmUnitDefault, 2, 4, false, 0},
    {"default-estep/4x4", 1, kEmUnitDefault, 4, 4, false, 0},
    {"big-estep/8x4", 1, kEmUnitBig, 8, 4, false, 0},
    {"big-estep/16x4", 1, kEmUnitBig, 16, 4, false, 0},
};
inline constexpr int kNumEmBuilds = sizeof(kEmBuilds) / sizeof(kEmBuilds[0]);

inline int em_chunks(int E) { return E <= 64 ? 1 : (E <= 128 ? 2 : (E <= 256 ? 4 : (E <= 512 ? 8 : 16))); }
inline int em_rows(int E) { return E <= 16 ? 1 : (E <= 32 ? 2 : 4); }  // BASELINE's `--bins 3,7,0.2` gives E = 23

// 0 = latency (max-ilp unit), 1 = latency (default unit), 2 = throughput: colate_em_kernel_variant's three values
inline int em_build_variant(const EmBuild& b) { return b.tput ? 2 : (b.unit == kEmUnitIlp ? 0 : 1); }

// The build of a launch of B replicates x E epochs on a device of `cus` compute units (0 = the query failed);
// forced: -1 = automatic, 0 / 1 / 2 = colate_em_force_variant's values (heeded for E <= 128 only).  Never NULL for
// 1 <= E <= 1024 and mode 0 or 1.
//
// Measured (tools/variant_sweep.sh, profiles/r02/variants.txt): since the steady-state loops the max-ilp unit's capped build
// fits 3 waves per SIMD as well (157 VGPRs) and is the faster latency build at every batch size (1.29 against 1.33 ms at
// B = 400); two 6-wave workgroups per CU beat the two-wave layout up to 2 x #CUs (B = 512: 1.30 against 2.09 ms),
// beyond that the throughput layout wins (B = 640: 2.09 against 2.12 ms; B = 1536: 2.70 against 3.65 ms).  The
// default unit's latency builds stay selectable (COLATE_EM_VARIANT=latency) for A/B runs.
inline const EmBuild* em_build_for(int mode, int B, int E, int cus, int forced) {
  EmBuild want{nullptr, mode, kEmUnitDefault, em_chunks(E), 4, false, 0};
  if (want.nch > 4) {  // 257 .. 1024 epochs: the two-wave layout, general loop only
    want.unit = kEmUnitBig;
    want.tput = mode == 0;
  } else if (mode == 0) {
    int variant = 2;  // 129 .. 256 epochs: only the two-wave layout fits the register file without scratch
    if (want.nch <= 2) variant = (forced >= 0 && forced <= 2) ? forced : ((cus <= 0 || B <= 2 * cus) ? 0 : 2);
    want.tput = variant == 2;
    if (variant == 0) want.unit = kEmUnitIlp;
    if (want.nch == 1) want.erows = em_rows(E);
    // the free build: every workgroup has a CU to itself, so the cap that keeps three waves per SIMD is not needed
    if (variant == 0 && want.nch == 1 && cus > 0 && B <= cus) want.wpe = 2;
  }
  for (const EmBuild& b : kEmBuilds)
    if (b.mode == want.mode && b.unit == want.unit && b.nch == want.nch && b.erows == want.erows && b.tput == want.tput &&
        b.wpe == want.wpe)
      return &b;
  return nullptr;
}

// colate_em_kernel_build_for, once for the library and for the host-only build (tools/no_device_stubs.cpp): checks the
// arguments, copies the build's name into name[cap] and returns its length; a negative value indexes kEmBuildErrors
inline constexpr int kEmBuildMaxEpochs = 1024;  // = COLATE_EM_MAX_E (em_kernels.h), COLATE_MAX_EPOCHS (colate_amd.h)
inline constexpr const char* kEmBuildErrors[] = {"", "bad mode or sizes for an EM kernel build", "name buffer too small"};
inline int em_build_copy_name(const EmBuild* b, char* name, int cap) {
  if (!b) return -1;
  const int n = (int)strlen(b->name);
  if (!name || cap <= n) return -2;
  memcpy(name, b->name, n + 1);
  return n;
}
inline int em_build_name_for(int mode, int B, int E, int cus, int forced, char* name, int cap) {
  if ((mode != 0 && mode != 1) || B < 0 || E < 1 || E > kEmBuildMaxEpochs) return -1;
  return em_build_copy_name(em_build_for(mode, B, E, cus, forced), name, cap);
}

// colate_em_kernel_builds: the names of the table's builds of `mode`, newline-separated; returns the length, or -2
// (kEmBuildErrors) if cap is too small
inline int em_build_names(int mode, char* buf, int cap) {
  if (!buf) return -2;
  int len = 0;
  for (const EmBuild& b : kEmBuilds) {
    if (b.mode != mode) continue;
    const int n = (int)strlen(b.name);
    if (len + n + 2 > cap) return -2;
    if (len) buf[len++] = '\n';
    memcpy(buf + len, b.name, n);
    len += n;
  }
  if (len + 1 > cap) return -2;
  buf[len] = 0;
  return len;
}
