// catan_teacher.h - what catan_abi.hip sees of catan_teacher.hip (kickstarting from the rule-based player).
//
// catan_teacher.hip is a translation unit of its own: its three kernels live in a SECOND gfx950 code object inside libcatan_hip.so, and
// the code object of catan_abi.hip - every kernel that runs when no teacher is configured - stays what it is without them.  The ABI's
// entry points (argument checks, the handle's fields) stand in catan_abi.hip and launch through these three functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace catan {

constexpr int IMIT_WORDS = 33, IMIT_PART = 30;       // the read-out block of k_imitation_loss; partial q of a workgroup = word q + 2
constexpr int IMIT_BLOCKS = 256, IMIT_THREADS = 256; // its grid is capped at IMIT_BLOCKS workgroups; workspace = IMIT_PART * IMIT_BLOCKS + 1 doubles

// records: the handle's game records (Ctx::R), n its games, mpk its side rows; busy: null outside a deferred sequence
hipError_t teacher_launch_complete(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                   int32_t* actions, hipStream_t stream);
hipError_t teacher_launch_label(long n, int T, const long long* n_act, const uint8_t* live, const long long* active_pid, const int32_t* deciding,
                                const uint8_t* waiting_before, const int32_t* labels, short* st_teacher, hipStream_t stream);
hipError_t teacher_launch_imitation(const float* lp, const long long* teacher, long B, float* loss, float* dlp, double* block, double* workspace,
                                    hipStream_t stream);

}  // namespace catan
