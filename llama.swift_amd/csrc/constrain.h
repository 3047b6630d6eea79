// constrain.h -- a token-level constraint (include/llamahip.h): the byte automaton a caller supplies, lifted once to the model's
// tokens.  The host half (constrain.cpp) is pure: it reads the handle's vocabulary through the public accessors and nothing else, so
// tools/host_sanitize compiles it as it is.  The device copy of the table is the driver's (llamahip.cpp): made by the first device call that
// uses the constraint, registered with the handle's DevOwner, released through `dev_release` by llamahip_constraint_free -- or by the handle's
// owner, which outlives no constraint: llamahip_model_free clears `dev` / `dev_release` of the constraints it still knows.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/llamahip.h"

struct llamahip_constraint {
    const llamahip_model *m = nullptr;      // the handle whose vocabulary the table was lifted on
    int32_t n_states = 0;                   // DONE included: rows of `next`
    int32_t n_vocab = 0;
    int32_t start = 0, stop_token = 0;
    std::vector<uint16_t> next;             // [n_states][n_vocab], LLAMAHIP_CONSTRAINT_BANNED = not allowed
    std::vector<int32_t> single;            // [n_states]: the state's single allowed token; -1 none allowed (DONE's entry: it yields nothing), -2 several
    // the device copy (null until a device call needs it) and how to release it
    uint16_t *dev = nullptr;
    void (*dev_release)(llamahip_constraint *) = nullptr;
};

namespace lh {
constexpr uint16_t DFA_BANNED = 0xFFFF;
constexpr int32_t DFA_STATES_MAX = 4096;                          // byte-states a caller may supply (DONE is one more row)
constexpr size_t DFA_TABLE_BYTES_MAX = (size_t) 256 << 20;
// the pick rule on one row: see llamahip_constraint_pick.  -1 where nothing is allowed
int32_t dfa_pick_row(const uint16_t *row, int32_t n_vocab, const float *logits);
}  // namespace lh
