// catan_trader.h - what catan_abi.hip sees of catan_trader.hip (the rule-based "trader" player).
//
// catan_trader.hip is a translation unit of its own, as catan_teacher.hip is: k_sample_trader lives in a gfx950 code object of its own
// inside libcatan_hip.so, and the code object of catan_abi.hip - every kernel that runs when the style is not selected - stays what it
// is without it.  The ABI's entry points (argument checks, the handle's counter block) stand in catan_abi.hip and launch through this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace catan {

// the counter block of the trader (catan_scripted_trade_counts): one uint64 each
enum { TC_DECISIONS = 0, TC_PROPOSALS = 1, TC_RESPONSES = 2, TC_ACCEPTS = 3, TC_REJECT_ILLEGAL = 4, TC_REJECT_OTHER = 5, TC_EXCHANGES = 6,
       TC_FALLBACKS = 7, TC_WORDS = 8 };

// records: the handle's game records (Ctx::R), n its games, mpk its side rows; busy: null outside a deferred sequence;
// counts: device uint64 [TC_WORDS]
hipError_t trader_launch_sample(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                int32_t* actions, unsigned long long* counts, hipStream_t stream);

}  // namespace catan
