// stamps.h -- the timeline instrumentation of the diagnostic build (-DCN_STAMPS): the stamp arrays that
// cn_debug_stamps() reads back and the STAMP_* macros, with their no-op forms for the shipped library. Needs nothing.
#pragma once

// Diagnostic build only (-DCN_STAMPS): per-workgroup s_memtime stamps at phase boundaries, read back
// with cn_debug_stamps(). The shipped library is built without it (no stamp executes).
#ifdef CN_STAMPS
#define CN_NSTAMP 24
__device__ unsigned long long cn_stamp_a[4096 * CN_NSTAMP];
__device__ unsigned long long cn_stamp_b[8192 * CN_NSTAMP];
__device__ unsigned long long cn_stamp_c[8192 * 4];   // crowded rejection: ensure / cand / test / passes
__device__ unsigned long long cn_stamp_p[8192 * 2];   // spawn waves: start / end of each env's latest spawn
__device__ unsigned long long cn_stamp_r[8192 * 2];   // every workgroup: start / end on the device-wide 100 MHz clock
__device__ unsigned long long cn_stamp_s[8192 * 16];   // spawn_env: start, seeded, robot, after human i (3 + i)
#define STAMP_S(e, k) do { if (lane == 0 && (e) >= 0 && (e) < 8192) cn_stamp_s[(e) * 16 + (k)] = clock64(); } while (0)
// every workgroup: where it ran (HW_REG_XCC_ID, HW_REG_HW_ID: CU / SE fields) and its start / end on its XCD's
// shader clock, so that its in-kernel clock is (x[3] - x[2]) / (r[1] - r[0]) x 100 MHz (tools/probe_stamps.py xcd)
__device__ unsigned long long cn_stamp_x[8192 * 4];
#ifndef CN_LABEL_ROT
#define CN_LABEL_ROT 0
#endif
#define CN_GETREG32(id) ((unsigned)__builtin_amdgcn_s_getreg((id) | (31 << 11)))
#define STAMP_R(k) do { if (threadIdx.x == 0 && blockIdx.x < 8192) { \
        if ((k) == 0) { cn_stamp_x[blockIdx.x * 4] = CN_GETREG32(20); cn_stamp_x[blockIdx.x * 4 + 1] = CN_GETREG32(4); } \
        cn_stamp_x[blockIdx.x * 4 + 2 + (k)] = __builtin_amdgcn_s_memtime(); \
        cn_stamp_r[blockIdx.x * 2 + (k)] = __builtin_amdgcn_s_memrealtime(); } } while (0)
// -DCN_STAMP_STEP=k: the stamps of cn_step_kernel's workgroups and of their phase-5 items record step k of a
// multi-step launch instead of its last step (which alone stores the outputs and computes the info row); the
// items of the other steps pass -1 for their env (STAMP_B, WRng::edbg)
#ifndef CN_STAMP_STEP
#define CN_STAMP_STEP -1
#endif
#define CN_STAMP_ON (CN_STAMP_STEP < 0 || step == CN_STAMP_STEP)
#define STAMP_A(k) do { const unsigned sb_ = (unsigned)sb; if (threadIdx.x == 0 && sb_ < 4096 && CN_STAMP_ON) cn_stamp_a[sb_ * CN_NSTAMP + (k)] = clock64(); } while (0)
#define STAMP_B(w, k) do { if ((threadIdx.x & 63) == 0 && (unsigned long long)(w) < 8192) cn_stamp_b[(w) * CN_NSTAMP + (k)] = clock64(); } while (0)
// stamp k by thread t (a lane of another wave than thread 0's)
#define STAMP_T(k, t) do { const unsigned sb_ = (unsigned)sb; if (threadIdx.x == (t) && sb_ < 4096 && CN_STAMP_ON) cn_stamp_a[sb_ * CN_NSTAMP + (k)] = clock64(); } while (0)
// phase 2 of the quad path per WAVE (lane 0 of each of the workgroup's four waves), [workgroup][wave][CN_NWSTAMP]:
// clocks at 0 lines + ranking done, 1 lp2_r done, 2 past the barrier before lp3_tasks, 3 lp3_tasks done,
// 4 lp3_replay + human_post done; then the linearProgram1 bodies the wave's linear programs ran (LpCount, orca_lp.h):
// 5 / 6 lp2_r's distinct line indices over the wave / largest count of one quad, 7 / 8 the same of lp3_tasks, summed
// over its rounds, 9 those rounds. Read back with cn_debug_stamps_w() (tools/probe_stamps.py phase2)
#define CN_NWSTAMP 16
__device__ unsigned long long cn_stamp_w[4096 * 4 * CN_NWSTAMP];
#define STAMP_WV(k, v) do { const unsigned sb_ = (unsigned)sb; if ((threadIdx.x & 63) == 0 && sb_ < 4096 && CN_STAMP_ON) cn_stamp_w[(sb_ * 4 + (threadIdx.x >> 6)) * CN_NWSTAMP + (k)] = (v); } while (0)
#define STAMP_W(k) STAMP_WV(k, clock64())
#else
#define CN_LABEL_ROT 0
#define CN_STAMP_ON true
#define STAMP_T(k, t) do { } while (0)
#define STAMP_W(k) do { } while (0)
#define STAMP_A(k) do { } while (0)
#define STAMP_B(w, k) do { } while (0)
#define STAMP_R(k) do { } while (0)
#define STAMP_S(e, k) do { } while (0)
#endif
