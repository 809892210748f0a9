// The refusal paths of the decimation entry points (include/rtgs_slam.h, "mesh decimation"): a null pointer that is needed
// or a count < 0 or >= 2^31 must return -1, and nothing to do must return 0, both before any launch - so this runs without a
// GPU.  A stand-alone host program for the sanitizers; from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         rtg_slam_amd/csrc/mesh_decimate.hip tools/probe/mesh_decimate_refusals.cpp -o tools/probe/mesh_decimate_refusals
//   tools/probe/mesh_decimate_refusals          # prints "0 failures", exit code 0
#include "../../include/rtgs_slam.h"
#include <stdio.h>
#include <stdint.h>
#include <math.h>
int main() {
  int bad = 0;
  float v[9] = {0}; int32_t f[3] = {0, 1, 2}; int64_t order[3] = {0, 1, 2}, start[4] = {0, 1, 2, 3}; double Q[33]; int32_t i32[4]; int64_t i64[4]; double d[4];
  const int64_t BIG = 1LL << 31;
#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { printf("FAIL %s -> %d, want %d\n", #call, rc_, (want)); ++bad; } } while (0)
  EXPECT(rtgs_mesh_decimate_quadrics(nullptr, f, 3, 1, order, start, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(v, nullptr, 3, 1, order, start, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(v, f, 3, 1, nullptr, start, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(v, f, 3, 1, order, nullptr, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(v, f, 3, 1, order, start, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(v, f, BIG, 1, order, start, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(v, f, 3, BIG, order, start, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(v, f, -1, 1, order, start, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_quadrics(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr), 0);
  EXPECT(rtgs_mesh_decimate_edge_keys(nullptr, 1, 3, i64, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_edge_keys(f, 1, 3, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_edge_keys(f, 1, 0, i64, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_edge_keys(f, BIG, 3, i64, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_edge_keys(f, 1, BIG, i64, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_edge_keys(nullptr, 0, 3, nullptr, nullptr), 0);
  EXPECT(rtgs_mesh_decimate_locks(nullptr, i64, 1, 3, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_locks(i64, nullptr, 1, 3, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_locks(i64, i64, 1, 3, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_locks(i64, i64, -1, 3, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_locks(i64, i64, 1, BIG, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_locks(i64, i64, 4 * BIG, 3, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_locks(nullptr, nullptr, 0, 3, nullptr, nullptr), 0);
  EXPECT(rtgs_mesh_decimate_propose(nullptr, f, 3, 1, order, start, i32, Q, 0.0, i32, d, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(v, f, 3, 1, order, start, nullptr, Q, 0.0, i32, d, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(v, f, 3, 1, order, start, i32, nullptr, 0.0, i32, d, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(v, f, 3, 1, order, start, i32, Q, 0.0, nullptr, d, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(v, f, 3, 1, order, start, i32, Q, 0.0, i32, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(v, f, 3, 1, order, start, i32, Q, NAN, i32, d, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(v, f, BIG, 1, order, start, i32, Q, 0.0, i32, d, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(v, f, 3, BIG, order, start, i32, Q, 0.0, i32, d, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_propose(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0.0, nullptr, nullptr, nullptr), 0);
  EXPECT(rtgs_mesh_decimate_claim(nullptr, order, start, i64, i32, 1, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_claim(f, order, start, i64, i32, 1, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_claim(f, order, start, i64, i32, BIG, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_claim(f, order, start, i64, i32, -1, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_claim(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr), 0);
  EXPECT(rtgs_mesh_decimate_select(f, order, start, i64, i32, 1, nullptr, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_select(f, order, start, i64, i32, 1, i32, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_select(f, order, start, nullptr, i32, 1, i32, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_select(f, order, start, i64, i32, BIG, i32, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_select(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr), 0);
  EXPECT(rtgs_mesh_decimate_apply(nullptr, i32, i32, 1, i32, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_apply(i64, i32, nullptr, 1, i32, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_apply(i64, i32, i32, 1, nullptr, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_apply(i64, i32, i32, 1, i32, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_apply(i64, i32, i32, BIG, i32, Q, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_apply(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr), 0);
  EXPECT(rtgs_mesh_decimate_reindex(nullptr, 1, i32, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_reindex(f, 1, nullptr, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_reindex(f, 1, i32, nullptr, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_reindex(f, BIG, i32, i32, nullptr), -1);
  EXPECT(rtgs_mesh_decimate_reindex(nullptr, 0, nullptr, nullptr, nullptr), 0);
  printf("%d failures\n", bad);
  return bad != 0;
}
