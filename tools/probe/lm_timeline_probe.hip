// Timeline of a wave of k_sba_lm's ROW instances: sba.hip compiled with ACS_LM_STAMPS, which makes
// those instances read s_memtime at entry, after the first and the last vector wait, at loop entry,
// at loop exit, and before and after the wait that precedes the final store; lane 0 of each wave
// stores the seven stamps and the wave's s_memrealtime span (100 MHz) as 8 words with ordinary
// vector stores. In the library's own build no stamp executes: the macro is defined here only.
//
// This file takes sba.hip's place in a diagnostic copy of the library (same C ABI plus
// acs_sba_lm_stamps), which tools/lm_timeline.py drives on the benchmark problem:
//   python -m acinoset_amd.build      # the objects of the other sources
//   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I include -Wno-unused-result \
//     -mllvm -amdgpu-kernarg-preload-count=16 -shared tools/probe/lm_timeline_probe.hip \
//     $(ls acinoset_amd/csrc/build/*.o | grep -v '/sba\.o') -o tools/probe/libacinoset_lm_timeline.so
//   ACINOSET_HIP_LIB=tools/probe/libacinoset_lm_timeline.so python tools/lm_timeline.py
#define ACS_LM_STAMPS 1
#include "../../acinoset_amd/csrc/sba.hip"

// Where the next ROW launches write their stamps: 8 words per wave (block), device memory; null = nowhere.
extern "C" int acs_sba_lm_stamps(unsigned long long* dev_words) {
  g_lm_stamps = dev_words;
  return 0;
}
