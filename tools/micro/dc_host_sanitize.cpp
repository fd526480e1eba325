// The deep-clustering 2-means host code (csrc/dc_run.inc) under the host sanitizers: a stand-alone program over the emulation build of
// the library (the product's translation unit against the mock HIP runtime of tests/emu).  From the repository root:
//   g++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I tests/emu/include -pthread \
//       onssen_amd/csrc/onssen_hip.hip tools/micro/dc_host_sanitize.cpp -o dc_host_sanitize && ./dc_host_sanitize
// Every DC entry at the smallest shapes: the size / offset queries, both forms of the clustering (uniform and ragged), the compacted
// route, and the refusals.  Workgroups run one after another here, so the persistent Lloyd launches give up their bounded waits
// (status word 1) -- the launch-per-iteration form is the one that completes.  Prints one line and exits 0; a sanitizer report aborts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/onssen_hip.h"

static void* ws_alloc(size_t nb, size_t head) {      // exactly nb bytes (so that a byte past the end is a report), 256-byte aligned
  void* p = aligned_alloc(256, (nb + 255) / 256 * 256);
  memset(p, 0xA5, nb);
  memset(p, 0, head);
  return p;
}

int main() {
  int bad = 0;
  onssen_xcd_spin_limit(2000);
  const int shapes[][4] = {{1, 1, 1, 3}, {1, 2, 3, 4}, {2, 3, 5, 20}, {3, 5, 9, 7}};
  for (const auto& s : shapes) {
    const int B = s[0], T = s[1], F = s[2], D = s[3];
    const size_t n = (size_t)B * T * F;
    std::vector<float> emb_raw(n * D + 4), feat(n), masks(n * 2);
    float* emb = emb_raw.data();
    while (reinterpret_cast<uintptr_t>(emb) & 15u) ++emb;
    for (size_t i = 0; i < n * D; ++i) emb[i] = (float)((i * 2654435761u >> 7) % 2001) / 1000.f - 1.f;
    for (size_t i = 0; i < n; ++i) feat[i] = (float)((i * 40503u >> 3) % 4001) / 1000.f - 3.f;
    std::vector<int32_t> frames(B);
    for (int b = 0; b < B; ++b) frames[b] = b == 1 ? 1 : T;
    size_t comp_off = 0, dest_off = 0;
    bad += onssen_dc_compact_layout(B, T, F, D, &comp_off, &dest_off) != 0;
    const size_t nb = onssen_dc_cluster_workspace_bytes(B, T, F, D), nbc = onssen_dc_compact_workspace_bytes(B, T, F, D);
    bad += !(onssen_dc_cluster_status_offset(B, D) < comp_off && comp_off < nb && nb <= dest_off && dest_off < nbc);
    for (int flags = 0; flags < 2; ++flags)
      for (int iters = 0; iters <= 3; iters += 3) {
        void* ws = ws_alloc(nb, comp_off);
        bad += onssen_dc_cluster_f32(emb, feat.data(), B, T, F, D, 40.f, iters, 1e-4f, masks.data(), ws, nb, flags, nullptr) != 0;
        memset(ws, 0, comp_off);
        bad += onssen_dc_cluster_ragged_f32(emb, feat.data(), B, T, frames.data(), F, D, 40.f, iters, 0.f, masks.data(), ws, nb, flags, nullptr) != 0;
        free(ws);
      }
    for (int ragged = 0; ragged < 2; ++ragged)
      for (int iters = 0; iters <= 3; iters += 3) {
        char* ws = (char*)ws_alloc(nbc, comp_off);
        bad += onssen_dc_index_f32(feat.data(), B, T, ragged ? frames.data() : nullptr, F, D, 40.f, ws, nbc, nullptr) != 0;
        memcpy(ws + comp_off, emb, n * D * sizeof(float));
        bad += onssen_dc_cluster_compact_f32(B, T, F, D, iters, 1e-4f, masks.data(), ws, nbc, 0, nullptr) != 0;
        free(ws);
      }
    // refusals: nothing is touched
    char* ws = (char*)ws_alloc(nbc, comp_off);
    bad += onssen_dc_cluster_f32(nullptr, feat.data(), B, T, F, D, 40.f, 3, 1e-4f, masks.data(), ws, nb, 0, nullptr) != ONSSEN_E_ARG;
    bad += onssen_dc_cluster_f32(emb, feat.data(), B, T, F, 33, 40.f, 3, 1e-4f, masks.data(), ws, nbc, 0, nullptr) != ONSSEN_E_ARG;
    bad += onssen_dc_cluster_f32(emb, feat.data(), B, T, F, D, 40.f, 3, 1e-4f, masks.data(), ws, nb - 1, 0, nullptr) != ONSSEN_E_WORKSPACE;
    bad += onssen_dc_cluster_f32(emb, feat.data(), B, T, F, D, 40.f, 3, 1e-4f, masks.data(), ws + 16, nb, 0, nullptr) != ONSSEN_E_ALIGN;
    bad += onssen_dc_cluster_ragged_f32(emb, feat.data(), B, T, nullptr, F, D, 40.f, 3, 1e-4f, masks.data(), ws, nb, 0, nullptr) != ONSSEN_E_ARG;
    bad += onssen_dc_index_f32(feat.data(), B, T, nullptr, F, D, 40.f, ws, nb, nullptr) != ONSSEN_E_WORKSPACE;
    bad += onssen_dc_index_f32(feat.data(), B, T, nullptr, F, D, 40.f, ws + 64, nbc, nullptr) != ONSSEN_E_ALIGN;
    bad += onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4f, masks.data(), ws, nbc, ONSSEN_DC_CLUSTER_LAUNCH_PER_ITERATION, nullptr) != ONSSEN_E_ARG;
    bad += onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4f, masks.data(), ws, nbc - 1, 0, nullptr) != ONSSEN_E_WORKSPACE;
    bad += onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4f, nullptr, ws, nbc, 0, nullptr) != ONSSEN_E_ARG;
    free(ws);
  }
  bad += onssen_dc_cluster_status_offset(0, 20) != 0 || onssen_dc_cluster_status_offset(3, 33) != 0;
  bad += onssen_dc_cluster_workspace_bytes(3, 0, 9, 20) != 0 || onssen_dc_compact_workspace_bytes(3, 5, 9, 0) != 0;
  bad += onssen_dc_compact_layout(3, 5, 0, 20, nullptr, nullptr) != ONSSEN_E_ARG;
  printf("dc_host_sanitize: %d unexpected return codes\n", bad);
  return bad != 0;
}
