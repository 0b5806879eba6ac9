// Masked GRU sequence kernels for the DSRNN policy.
//
// The reference runs its three GRUs (srnn_model.py:52-104, RNNBase._forward_gru) as torch nn.GRU calls over
// the segments between episode starts; every segment boundary re-enters cuDNN/MIOpen with the hidden state
// multiplied by the mask. Here a sequence of T steps is:
//   gi  = x @ W_ih^T + b_ih            one GEMM over all T*B rows (hipBLASLt, from the torch wrapper)
//   per step t:
//     gh = hm_t @ W_hh^T + b_hh        one GEMM (B x H -> B x 3H)
//     cn_gru_fwd_step                  gates + new state + the next step's masked state, one pass
//   backward, per step t (reversed):
//     cn_gru_bwd_step                  gate gradients from the saved gates, one pass
//     acc += dgh_t @ W_hh              one GEMM
//   then dW_ih, dW_hh, db_*, dx as single GEMMs / reductions over all T*B rows.
// Gate math and operation order follow ATen's GRU cell (the reference's nn.GRU):
//   r = sigmoid(gh_r + gi_r), z = sigmoid(gh_z + gi_z), n = tanh(gi_n + r * gh_n), h' = (h - n) * z + n.
// Memory-bound elementwise work: each thread handles 4 consecutive hidden units (16-byte accesses).
//
// The unit also holds the rest of the policy's kernels (PPO, attention, weight gradients). Everything is a section of
// this one translation unit in policy/*.h, listed below.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

#include "../../include/crowdnav.h"
#include "cn_host.h"

// ------------------------------------------------------------------------------------------------
// The kernels by topic. The order below is the kernels' order in the code object (the non-template ones; the
// templates' instantiations follow in the order policy_api.h first launches them), which is kept as tuned:
// hence the PPO kernels in two sections.
// ------------------------------------------------------------------------------------------------
#include "policy/gru_cell.h"       // sigm, CN_GATE / CN_GBWD, cn_gru_fwd / bwd / bwd_bias kernels, the bias reductions
#include "policy/gru_fused.h"      // GfSeg / GfArgs / GbSeg / GbArgs, cn_gru_fused_kernel, cn_gru_bwd_fused_kernel
#include "policy/ppo_act.h"        // cn_gaussian_act_kernel
#include "policy/gru_splitk.h"     // cn_gru_fused_sk_kernel, cn_gru_bwd_sk_kernel, device_cus, use_split_k, row_tile
#include "policy/ppo_gae.h"        // cn_gae_kernel
#include "policy/attn_pool.h"      // cn_attn_pool_fwd_kernel, cn_attn_pool_bwd_kernel
#include "policy/spatial_attn.h"   // cn_spatial_attn_fwd / bwd kernels and the _var pair
#include "policy/wgrad.h"          // cn_wgrad_part_kernel, cn_wgrad_sum_kernel, wgrad_grid
#include "policy/policy_api.h"     // extern "C": the functions of include/crowdnav.h served by this unit
