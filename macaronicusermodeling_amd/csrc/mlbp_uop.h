// The micro-op words of the lean X = 64 kernel (mlbp_lean_device.h), shared by the host compiler that writes them
// (build_lean_program, mlbp_compile.cpp) and the device code that reads them.  Plain constants and no include: the device header
// is also compiled at run time (mlbp_lean_jit.cpp), where no host header is at hand.
#ifndef MLBP_UOP_H
#define MLBP_UOP_H

namespace mlbp {
// micro-op word 0
constexpr int UOP_VAR = 1;          // bit 0: variable product only (stored, no contraction)
constexpr int UOP_MT = 2;           // bit 1: out = m^T . T (else T . m)
constexpr int UOP_PSLOT_SHIFT = 2;  // bits 2-4: pair slot (register-resident table; 0..7)
constexpr int UOP_NOP = 32;         // bit 5: empty second slot of a bundle
constexpr int UOP_STORE_VF = 64;    // bit 6: the variable->factor message is stored (word 5)
constexpr int UOP_NSRC_SHIFT = 8;   // bits 8-11: number of sources (1..4)
constexpr int UOP_CARRY_IN = 0x1000;   // a link of a long variable product: starts from the running product in registers
constexpr int UOP_CARRY_OUT = 0x2000;  // ... and hands it on instead of storing it
// micro-op words: 0 flags | 1-4 source byte offsets | 5 byte offset of the variable->factor message to store, or -1 |
// 6 destination byte offset | 7 unused.  Source words past the count hold the all-ones ext slot.
// A bundle = two micro-ops = 16 words = one s_load_dwordx16.
}  // namespace mlbp

#endif
