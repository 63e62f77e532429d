// catan_ppo.hip - fused GAE and clipped-PPO loss (forward + backward) kernels.
//
//   k_gae            BatchProcessor.compute_advantages_alt, the reverse-time recurrence of
//                    RL/ppo/process_batch.py:134-141 (one lane per game, coalesced [t][n] rows)
//   k_adv_stats/k_adv_normalise   the global normalisation of process_batch.py:142 (mean / unbiased std over T*N;
//                    exposed as (sum, sumsq, count) so that N>1 ranks can all-reduce three scalars - SURVEY 8(e))
//   k_ppo_loss       RL/ppo/ppo.py:46-48 (value normaliser) + :54-66 (loss) and its analytic gradient w.r.t.
//                    action_log_probs and values in the same pass
//   k_ppo_diag       opt-in read-out of what that loss did to a step's rows (approximate KL, clip counts, the sums behind the
//                    explained variance, the step's entropy and gradient norm), accumulated into one block of doubles per epoch
// fp32 recurrences are evaluated in the reference's operand order with contraction disabled (#pragma clang fp contract(off))
// so returns match torch bit-for-bit; reductions accumulate in fp64 in a fixed order (deterministic).
#include <hip/hip_runtime.h>

namespace catan {

constexpr int GAE_BLOCK = 256;

// rewards [T][N], values [T+1][N] (denormalised), masks [T+1][N] -> returns [T][N], adv_raw [T][N];
// partial [2 * gridDim.x] = per-block (sum, sumsq) of adv_raw in fp64
__global__ __launch_bounds__(GAE_BLOCK) void k_gae(const float* __restrict__ rewards, const float* __restrict__ values,
                                                   const float* __restrict__ masks, long T, long N, float gamma, float gl,
                                                   float* __restrict__ returns, float* __restrict__ adv, double* __restrict__ partial) {
    __shared__ double sh[2][GAE_BLOCK];
    const long n = (long)blockIdx.x * GAE_BLOCK + threadIdx.x;
    double sum = 0.0, sumsq = 0.0;
    if (n < N) {
        float gae = 0.0f;
        float v1 = values[T * N + n];
        for (long t = T - 1; t >= 0; t--) {
            const float m1 = masks[(t + 1) * N + n], v0 = values[t * N + n], r = rewards[t * N + n];
            float ret, a;
            {
                // every product rounded before it is added, as torch's separate operations do (the __fmul_rn / __fadd_rn of the HIP
                // headers are a plain * and +, which the default -ffp-contract fuses into v_fma_f32: the pragma is what forbids it)
#pragma clang fp contract(off)
                const float delta = (r + (gamma * v1) * m1) - v0;       // delta = r + gamma * v1 * m1 - v0          (process_batch.py:137)
                gae = delta + (gl * m1) * gae;                          // gae = delta + gamma * lambda * m1 * gae   (process_batch.py:138)
                ret = gae + v0;                                         // process_batch.py:139
                a = ret - v0;                                           // process_batch.py:141
            }
            returns[t * N + n] = ret;
            adv[t * N + n] = a;
            sum += (double)a; sumsq += (double)a * (double)a;
            v1 = v0;
        }
    }
    sh[0][threadIdx.x] = sum; sh[1][threadIdx.x] = sumsq;
    __syncthreads();
    for (int s = GAE_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) { sh[0][threadIdx.x] += sh[0][threadIdx.x + s]; sh[1][threadIdx.x] += sh[1][threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = sh[0][0]; partial[2 * blockIdx.x + 1] = sh[1][0]; }
}
// stats[3] = (sum, sumsq, count) from the per-block partials, fixed order
__global__ __launch_bounds__(GAE_BLOCK) void k_adv_stats(const double* __restrict__ partial, int nblocks, double count, double* __restrict__ stats) {
    __shared__ double sh[2][GAE_BLOCK];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += GAE_BLOCK) { a += partial[2 * i]; b += partial[2 * i + 1]; }
    sh[0][threadIdx.x] = a; sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = GAE_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) { sh[0][threadIdx.x] += sh[0][threadIdx.x + s]; sh[1][threadIdx.x] += sh[1][threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { stats[0] = sh[0][0]; stats[1] = sh[1][0]; stats[2] = count; }
}
// adv = (adv - mean) / (std_unbiased + 1e-5)   (process_batch.py:142); stats = GLOBAL (sum, sumsq, count)
__global__ __launch_bounds__(GAE_BLOCK) void k_adv_normalise(float* __restrict__ adv, long total, const double* __restrict__ stats) {
    const double cnt = stats[2], mean = stats[0] / cnt;
    const double var = (stats[1] - cnt * mean * mean) / (cnt - 1.0);
    const float fm = (float)mean, fs = (float)(sqrt(var > 0.0 ? var : 0.0)) + 1e-5f;
    for (long i = (long)blockIdx.x * GAE_BLOCK + threadIdx.x; i < total; i += (long)gridDim.x * GAE_BLOCK)
        adv[i] = (adv[i] - fm) / fs;
}

struct PpoArgs { float clip, value_coef, norm_mean, norm_std; int use_norm; };
// losses[0] = action loss, losses[1] = value loss (means over B = T*N/num_mini_batch rows, 2 000 .. ~2*10^5);
// d_logp / d_values = gradient of value_coef * L_v + L_pi (upstream gradient 1).  PPO_BLOCKS workgroups stream their share of
// the rows (24 B read + 8 B written per row); the per-workgroup fp64 partial sums go to `ws` and the workgroup that arrives
// last adds them up in index order, so the result does not depend on the schedule (ws: 2 * PPO_BLOCKS + 1 doubles, the last
// one the arrival counter - zero before the first call, left zero by every call).
constexpr int PPO_BLOCKS = 256, PPO_THREADS = 256;
static_assert(PPO_BLOCKS <= PPO_THREADS, "the last workgroup reduces one partial sum per lane");
__global__ __launch_bounds__(PPO_THREADS) void k_ppo_loss(const float* __restrict__ logp, const float* __restrict__ old_logp,
                                                          const float* __restrict__ adv, const float* __restrict__ values,
                                                          const float* __restrict__ old_values, const float* __restrict__ returns,
                                                          long B, PpoArgs a, float* __restrict__ losses,
                                                          float* __restrict__ d_logp, float* __restrict__ d_values, double* __restrict__ ws) {
    __shared__ double sh[2][PPO_THREADS];
    __shared__ bool last;
    double la = 0.0, lv = 0.0;
    const float invB = 1.0f / (float)B;
    const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
    for (long i = (long)blockIdx.x * PPO_THREADS + threadIdx.x; i < B; i += (long)gridDim.x * PPO_THREADS) {
        float vp = old_values[i], ret = returns[i];
        if (a.use_norm) { vp = (vp - a.norm_mean) / (a.norm_std + 1e-4f); ret = (ret - a.norm_mean) / (a.norm_std + 1e-4f); }   // ppo.py:46-48
        const float ratio = expf(logp[i] - old_logp[i]);                    // ppo.py:54
        const float ad = adv[i];
        const float s1 = ratio * ad;                                        // :55
        // torch.clamp / min / max pass NaN on where fminf / fmaxf return the other operand: a non-finite row reaches both the loss and
        // its own gradient (the comparisons below are false for NaN, so the ternaries keep it); finite rows take the same values as before
        const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
        const float s2 = rc * ad;                                           // :56
        const float smin = (s1 != s1 || s2 != s2) ? s1 + s2 : fminf(s1, s2);
        la += (double)(-smin);                                              // :57
        const bool inside = ratio >= lo && ratio <= hi;
        d_logp[i] = smin != smin ? smin : ((s1 <= s2 || inside) ? -s1 * invB : 0.0f);   // d(-min)/dlogp = -ratio * adv on the active branch
        const float v = values[i];
        const float dv = v - vp;
        const float vc = vp + (dv < -a.clip ? -a.clip : (dv > a.clip ? a.clip : dv));   // :59-60
        const float e1 = v - ret, e2 = vc - ret;
        const float l1 = e1 * e1, l2 = e2 * e2;                             // :61-62
        const float lmax = (l1 != l1 || l2 != l2) ? l1 + l2 : fmaxf(l1, l2);
        lv += 0.5 * (double)lmax;                                           // :63
        const bool vin = dv >= -a.clip && dv <= a.clip;
        // on a tie torch's maximum hands half of the gradient to each side, and the clipped side passes its half on only inside the range
        const float e2v = vin ? e2 : 0.0f;
        d_values[i] = lmax != lmax ? lmax : a.value_coef * invB * (l1 > l2 ? e1 : (l1 < l2 ? e2v : 0.5f * (e1 + e2v)));
    }
    sh[0][threadIdx.x] = la; sh[1][threadIdx.x] = lv;
    __syncthreads();
    for (int s = PPO_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) { sh[0][threadIdx.x] += sh[0][threadIdx.x + s]; sh[1][threadIdx.x] += sh[1][threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = sh[0][0]; ws[PPO_BLOCKS + blockIdx.x] = sh[1][0];
        __threadfence();
        unsigned long long* counter = reinterpret_cast<unsigned long long*>(ws + 2 * PPO_BLOCKS);
        last = atomicAdd(counter, 1ull) == (unsigned long long)gridDim.x - 1;
    }
    __syncthreads();
    if (last) {                                             // the whole last workgroup: partial k at lane k, then the same tree as above
        __threadfence();
        const bool have = threadIdx.x < gridDim.x;
        sh[0][threadIdx.x] = have ? __hip_atomic_load(&ws[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        sh[1][threadIdx.x] = have ? __hip_atomic_load(&ws[PPO_BLOCKS + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        __syncthreads();
        for (int s2 = PPO_THREADS / 2; s2 > 0; s2 >>= 1) {
            if (threadIdx.x < s2) { sh[0][threadIdx.x] += sh[0][threadIdx.x + s2]; sh[1][threadIdx.x] += sh[1][threadIdx.x + s2]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            losses[0] = (float)(sh[0][0] / (double)B); losses[1] = (float)(sh[1][0] / (double)B);
            *reinterpret_cast<unsigned long long*>(ws + 2 * PPO_BLOCKS) = 0ull;
        }
    }
}

// Diagnostics of one optimiser step of PPO.update (what the clipped objective of k_ppo_loss did to the step's rows), ACCUMULATED into a
// caller-owned block of PPO_DIAG_WORDS doubles - one block per epoch, zeroed by the caller, read by the host once per update.  Same
// inputs as k_ppo_loss (24 B read per row, nothing written per row) plus two optional device scalars (the step's entropy, the step's
// gradient norm).  Words (sums over the rows unless stated; d = (double)logp - (double)old_logp):
//    0 rows                     1 steps (+1 per call)        2 sum(-d)                    3 sum(expm1(d) - d), in fp64
//    4 max(d, 0)                5 max(-d, 0)                 6 ratio outside [lo, hi]     7 policy gradient zeroed (outside, s1 > s2)
//    8 |v - vp| > clip          9 value gradient zeroed (l2 > l1, not vin)               10, 11 sum ret, ret^2
//   12, 13 sum e, e^2 (e = ret - v)                          14, 15 sum e0, e0^2 (e0 = ret - vp)
//   16 sum entropy             17 sum gradient norm         18 steps with norm > max_grad_norm (never when that is <= 0)   19 max norm
// Words 6..9 classify with k_ppo_loss's own fp32 expressions (they count what the loss did); the sums are fp64 of the fp32 inputs, vp and
// ret normalised in fp64.  Up to PPO_BLOCKS workgroups keep fp64 partials in `ws` (PPO_DIAG_PART * PPO_BLOCKS + 1 doubles, the last one
// the arrival counter; zero before the first call, left zero by every call); the workgroup that arrives last folds them in index order
// and is the ONLY writer of the block: no atomic on the block, the same sequence of calls gives the same bits - as long as all calls
// into one block are on ONE stream (launches of one stream are ordered; two streams would race on the block's read-modify-write).
struct PpoDiagArgs { float clip, norm_mean, norm_std, max_grad_norm; int use_norm; };
constexpr int PPO_DIAG_WORDS = 20, PPO_DIAG_PART = 14;          // partial q of a workgroup = word q + 2
__device__ __forceinline__ bool ppo_diag_is_max(int q) { return q == 2 || q == 3; }
__device__ __forceinline__ void ppo_diag_tree(double (*sh)[PPO_THREADS]) {
    for (int s = PPO_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
#pragma unroll
            for (int q = 0; q < PPO_DIAG_PART; q++) {
                const double x = sh[q][threadIdx.x], y = sh[q][threadIdx.x + s];
                sh[q][threadIdx.x] = ppo_diag_is_max(q) ? fmax(x, y) : x + y;
            }
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(PPO_THREADS) void k_ppo_diag(const float* __restrict__ logp, const float* __restrict__ old_logp,
                                                          const float* __restrict__ adv, const float* __restrict__ values,
                                                          const float* __restrict__ old_values, const float* __restrict__ returns,
                                                          long B, PpoDiagArgs a, const float* __restrict__ entropy,
                                                          const float* __restrict__ grad_norm, double* __restrict__ block,
                                                          double* __restrict__ ws) {
    __shared__ double sh[PPO_DIAG_PART][PPO_THREADS];
    __shared__ bool last;
    double acc[PPO_DIAG_PART];
#pragma unroll
    for (int q = 0; q < PPO_DIAG_PART; q++) acc[q] = 0.0;
    const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
    const double nm = (double)a.norm_mean, ns = (double)a.norm_std + 1e-4;
    for (long i = (long)blockIdx.x * PPO_THREADS + threadIdx.x; i < B; i += (long)gridDim.x * PPO_THREADS) {
        const float lpi = logp[i], oli = old_logp[i], v = values[i], vp0 = old_values[i], ret0 = returns[i], ad = adv[i];
        // ---- what k_ppo_loss decided for the row: its fp32 expressions, unchanged
        float vp = vp0, ret = ret0;
        if (a.use_norm) { vp = (vp - a.norm_mean) / (a.norm_std + 1e-4f); ret = (ret - a.norm_mean) / (a.norm_std + 1e-4f); }
        const float ratio = expf(lpi - oli);
        const float s1 = ratio * ad;
        const float rc = fminf(fmaxf(ratio, lo), hi);
        const float s2 = rc * ad;
        const bool inside = ratio >= lo && ratio <= hi;
        const float dv = v - vp;
        const float vc = vp + fminf(fmaxf(dv, -a.clip), a.clip);
        const float e1 = v - ret, e2 = vc - ret;
        const float l1 = e1 * e1, l2 = e2 * e2;
        const bool vin = dv >= -a.clip && dv <= a.clip;
        acc[4] += inside ? 0.0 : 1.0;
        acc[5] += (!inside && s1 > s2) ? 1.0 : 0.0;
        acc[6] += vin ? 0.0 : 1.0;
        acc[7] += (!(l1 >= l2) && !vin) ? 1.0 : 0.0;
        // ---- the sums: fp64 of the fp32 inputs
        const double d = (double)lpi - (double)oli;
        acc[0] -= d;
        acc[1] += expm1(d) - d;
        acc[2] = fmax(acc[2], d);
        acc[3] = fmax(acc[3], -d);
        double vpd = (double)vp0, rd = (double)ret0;
        if (a.use_norm) { vpd = (vpd - nm) / ns; rd = (rd - nm) / ns; }
        const double e = rd - (double)v, e0 = rd - vpd;
        acc[8] += rd;  acc[9] += rd * rd;
        acc[10] += e;  acc[11] += e * e;
        acc[12] += e0; acc[13] += e0 * e0;
    }
#pragma unroll
    for (int q = 0; q < PPO_DIAG_PART; q++) sh[q][threadIdx.x] = acc[q];
    __syncthreads();
    ppo_diag_tree(sh);
    unsigned long long* counter = reinterpret_cast<unsigned long long*>(ws + PPO_DIAG_PART * PPO_BLOCKS);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < PPO_DIAG_PART; q++) ws[q * PPO_BLOCKS + blockIdx.x] = sh[q][0];
        __threadfence();
        last = atomicAdd(counter, 1ull) == (unsigned long long)gridDim.x - 1;
    }
    __syncthreads();
    if (last) {                                             // the whole last workgroup: partial k at lane k, the same tree; the partials go back to zero
        __threadfence();
        const bool have = threadIdx.x < gridDim.x;
#pragma unroll
        for (int q = 0; q < PPO_DIAG_PART; q++) {
            double* p = ws + q * PPO_BLOCKS + threadIdx.x;
            sh[q][threadIdx.x] = have ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;    // (0 is neutral for the two maxima too: they are >= 0)
            if (have) *p = 0.0;
        }
        __syncthreads();
        ppo_diag_tree(sh);
        if (threadIdx.x == 0) {
            block[0] += (double)B; block[1] += 1.0;
#pragma unroll
            for (int q = 0; q < PPO_DIAG_PART; q++) block[q + 2] = ppo_diag_is_max(q) ? fmax(block[q + 2], sh[q][0]) : block[q + 2] + sh[q][0];
            if (entropy) block[16] += (double)entropy[0];
            if (grad_norm) {
                const float g = grad_norm[0];
                block[17] += (double)g;
                if (a.max_grad_norm > 0.0f && g > a.max_grad_norm) block[18] += 1.0;
                block[19] = fmax(block[19], (double)g);
            }
            *counter = 0ull;
        }
    }
}

}  // namespace catan
