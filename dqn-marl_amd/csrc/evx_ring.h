// The uniform replay ring (evx_replay; DQNAgent.memory, agents/dqn_agent.py:88-99), each piece
// written once: what a push stores, the five-array row gather, the keyed draw with its slot
// mappings, the n-step chain, and the host-side argument checks the entries share. Used by
// csrc/replay.hip (every uniform-ring entry), csrc/env_step.hip (the fused orders + push + sample
// launch) and csrc/prio.hip (the prioritized sampler's row gather).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "evacx.h"
#include "evx_draws.h"
#include "evx_host.h"

namespace evxr {

// The sources of a push: one row per agent, the team reward / done flag per env.
struct push_src {
    const evx_obs *s, *s2, *s2_term;
    const int32_t* a;
    const double* r_env;
    const uint8_t* done_env;
};
// Five arrays of transitions: a ring's (an evx_replay without its capacity) or a batch's.
struct rows {
    evx_obs *s, *s2;
    int32_t* a;
    float* r;
    uint8_t* done;
};

// What a push gives source row `row` of env e, as element k of dst: the agent's own s / a, the
// terminal observation where the env is done (auto-reset: s2 is already the next episode's), and
// the env's team reward (f32) and done flag. I: the caller's env index type (the single rings' is
// an int quotient, and stays one).
template <class I>
__device__ __forceinline__ void push_row(const push_src& p, int64_t row, I e, const rows& dst, int64_t k) {
    dst.s[k] = p.s[row];
    dst.s2[k] = (p.s2_term && p.done_env[e]) ? p.s2_term[row] : p.s2[row];
    dst.a[k] = p.a[row];
    dst.r[k] = (float)p.r_env[e];
    dst.done[k] = p.done_env[e];
}
// DQNAgent.remember: source row `row` of env e into ring element `slot`.
template <class I>
__device__ __forceinline__ void ring_put(const evx_replay& rp, int64_t slot, const push_src& p, int64_t row, I e) {
    push_row(p, row, e, rows{rp.s, rp.s2, rp.a, rp.r, rp.done}, slot);
}
// Ring element j into row i of out.
__device__ __forceinline__ void ring_take(const evx_replay& rp, int64_t j, const rows& out, int64_t i) {
    out.s[i] = rp.s[j];
    out.s2[i] = rp.s2[j];
    out.a[i] = rp.a[j];
    out.r[i] = rp.r[j];
    out.done[i] = rp.done[j];
}

// Sampling WITHOUT replacement, as DQNAgent.learn's random.sample(memory, B)
// (agents/dqn_agent.py:132): draw i of a batch is perm(i) for a keyed pseudo-random permutation
// perm of [0, n) -- a 6-round balanced Feistel network on the smallest even-width domain 2^w >= n,
// cycle-walked back into [0, n) (terminates: i's cycle under the domain permutation contains i
// itself; expected < 4 rounds of walking since 2^w < 4n). Round keys from Philox4x32-10 of the
// draw's (offset, stream) under the seed, so each learn step's batch is a fresh permutation and
// the B draws are distinct (B <= n). oracle/draw_oracle.c orc_replay_indices restates it.
__device__ __forceinline__ int64_t perm_draw(uint64_t n, uint64_t seed, uint64_t offset, uint32_t stream, int i) {
    const evxd::perm_key pk = evxd::make_perm_key(n, seed, offset, stream);
    return (int64_t)evxd::perm_apply(pk, (uint64_t)i, n);
}

// Where draw i of grid row g lands:
//   WINDOW  one ring, the `size` slots from `base` on, wrapped (base 0: the whole ring)
//   AGENTS  one ring of `nets` interleaved agents: agent g's own transitions, the slots == g (mod
//           nets), under a permutation keyed by the agent; joint: one permutation for every agent
//           (the same env-steps)
//   BLOCKS  ring g of [nets][capacity], WINDOW's draws over [0, size) under (seed, offset + g B)
// Every mapping writes batch row g B + i; the slot is local to its ring, which starts
// draw_ring<MAP>() elements into the arrays.
enum { WINDOW, AGENTS, BLOCKS };
struct draw_args {
    int64_t base, size;
    int B, nets, joint;
    uint64_t seed, offset;
};
template <int MAP>
__device__ __forceinline__ int64_t draw_slot(const draw_args& d, int64_t C, int i, int g) {
    if (MAP == AGENTS) {
        const uint32_t stream = d.joint ? 0u : (uint32_t)g;
        return perm_draw((uint64_t)(d.size / d.nets), d.seed, d.offset, stream, i) * d.nets + g;
    }
    if (MAP == BLOCKS) return perm_draw((uint64_t)d.size, d.seed, d.offset + (uint64_t)g * (uint64_t)d.B, 0u, i);
    int64_t j = d.base + perm_draw((uint64_t)d.size, d.seed, d.offset, 0u, i);
    if (j >= C) j -= C;
    return j;
}
template <int MAP>
__device__ __forceinline__ int64_t draw_ring(int64_t C, int g) {
    return MAP == BLOCKS ? (int64_t)g * C : 0;
}

// n-step row of local slot j0 of the ring at element offset `ring` (evx_replay_nstep; not the
// reference's, whose target is one step deep). Every training step pushes `stride` rows in the same
// order, so the successor of slot j (same env, same robot, next env step) is slot (j + stride) mod
// capacity while that slot lies in the live range [base, base + count) mod capacity (push order,
// oldest first): no link array. The chain stops at n_step links, at a terminal slot (so never
// across an auto-reset: that slot's s2 is the terminal observation) or at the end of the range; a
// slot outside the range keeps its own row (L = 1). All f32; R + g * r stays a multiply and an add
// (-ffp-contract=off); int64 slot arithmetic. j0 < capacity and every later slot is taken mod
// capacity: nothing is read outside the ring.
__device__ __forceinline__ void ring_chain(const evx_replay& rp, int64_t ring, int64_t j0, int64_t base, int64_t count,
                                           int64_t stride, int n_step, float gamma, int64_t i, float* r,
                                           float* gamma_row, uint8_t* done, evx_obs* s2, int32_t* len) {
    const int64_t C = rp.capacity;
    int64_t d0 = j0 - base;
    if (d0 < 0) d0 += C;
    int64_t j = j0;
    float R = rp.r[ring + j0], g = gamma;
    uint8_t dn = rp.done[ring + j0];
    int L = 1;
    while (L < n_step && !dn && d0 + (int64_t)L * stride < count) {
        j = (j0 + (int64_t)L * stride) % C;
        R = R + g * rp.r[ring + j];
        g = g * gamma;
        dn = rp.done[ring + j];
        L++;
    }
    r[i] = R;
    gamma_row[i] = g;
    done[i] = dn;
    s2[i] = rp.s2[ring + j];
    if (len) len[i] = L;
}

// ------------------------------------------------------------------ host-side argument checks
// Each takes the entry's name and leaves the refusal in evxh's error text; 0: passed.
using evxh::failf;

static inline int ring_arrays_ok(const char* who, const evx_replay* rp) {
    return !rp->s || !rp->s2 || !rp->a || !rp->r || !rp->done ? failf(-22, "%s: NULL ring array", who) : 0;
}

// A draw of B rows per agent from a ring of `nets` interleaved agents (the AGENTS mapping).
static inline int agents_ok(const char* who, const evx_replay* rp, int64_t size, int32_t B, int32_t nets, bool joint) {
    if (nets < 1 || nets > 65535) return failf(-22, "%s: nets must be 1..65535", who);
    if (rp->capacity % nets) return failf(-22, "%s: capacity must be a multiple of nets", who);
    if (size < nets || size > rp->capacity || size % nets)
        return failf(-22, "%s: size must be a positive multiple of nets within the capacity", who);
    if (B > size / nets)
        return failf(-22, "%s: sample larger than %s population", who, joint ? "the" : "an agent's");
    return 0;
}

// The chain arguments of the single-ring entries, in the order they test them. On success *stride is
// clamped: a stride beyond the ring never finds a successor inside the range (count <= capacity), so
// the capacity stands for it and L * stride cannot overflow.
static inline int chain_ok(const char* who, const evx_replay* rp, int64_t base, int64_t count, int64_t* stride,
                           int32_t n_step, float gamma) {
    if (n_step < 1 || n_step > EVX_NSTEP_MAX) return failf(-22, "%s: n_step must be 1..EVX_NSTEP_MAX (32)", who);
    if (*stride < 1) return failf(-22, "%s: stride must be >= 1", who);
    if (count < 0 || count > rp->capacity) return failf(-22, "%s: count must lie in [0, capacity]", who);
    if (base < 0 || base >= rp->capacity) return failf(-22, "%s: base must lie in [0, capacity)", who);
    if (!std::isfinite(gamma)) return failf(-22, "%s: gamma must be finite", who);
    *stride = std::min<int64_t>(*stride, rp->capacity);
    return 0;
}
// The block rings' entry: its own order and wording of the range, a depth and a discount per ring; the
// same clamp.
static inline int chain_blocks_ok(const char* who, const evx_replay* rp, int64_t base, int64_t count, int64_t* stride,
                                  const int32_t* n_step, const float* gamma, int rings) {
    if (count < 0 || count > rp->capacity) return failf(-22, "%s: count outside [0, capacity]", who);
    if (base < 0 || base >= rp->capacity) return failf(-22, "%s: base outside [0, capacity)", who);
    if (*stride < 1) return failf(-22, "%s: stride must be >= 1", who);
    for (int k = 0; k < rings; k++) {
        if (n_step[k] < 1 || n_step[k] > EVX_NSTEP_MAX) return failf(-22, "%s: n_step must be 1..EVX_NSTEP_MAX (32)", who);
        if (!std::isfinite(gamma[k])) return failf(-22, "%s: gamma must be finite", who);
    }
    *stride = std::min<int64_t>(*stride, rp->capacity);
    return 0;
}

}  // namespace evxr
