// What the recurrent inference kernels share, stated once: the fp16 families of lstm.hip and the 8-bit kernel of lstm_q8.hip. The exchange
// protocol - the part whose mistakes are hangs, not wrong numbers - lives here next to the argument for why it is safe; the kernels keep
// their schedules (where a poll, a DMA, a barrier or a wait is issued) and call these functions for what they issue there.
//
// Geometry of the "four slices of one ring per workgroup" kernels (wgx, wgx2, wide, q8): a ring is 16 chunks (one MFMA column tile), a
// wave owns one slice of U = 4 * MT hidden units of it, wave w polls k-steps w, w + 4, .. of the ring's h tile and moves k-steps 3 - w,
// 7 - w, .. of the x stream. A tile is [k-step][lane][16 bytes]: ready-made MFMA B fragments.
#pragma once
#include "common.h"

namespace bh {

// ---- 1. the exchange sentinel ---------------------------------------------------------------------------------------------------------
// fp16: the buffer is armed with 0xFFFF; |h| <= 1 never has bit 14 set, so one OR-reduction + one mask test validates eight halves.
constexpr unsigned SENTINEL_MASK = 0x40004000u;
__device__ __forceinline__ bool armed_f16(const uint4_t& v) { return ((v.x | v.y | v.z | v.w) & SENTINEL_MASK) != 0; }
// int8: armed with 0x80 (-128 is not a quantised value): any byte of the four words equal to 0x80?  (x ^ 0x80 has a zero byte)
__device__ __forceinline__ bool has_sentinel(const uint4_t& v) {
    unsigned r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned y = v[i] ^ 0x80808080u;
        r |= (y - 0x01010101u) & ~y & 0x80808080u;
    }
    return r != 0;
}

__device__ __forceinline__ int xcc_id() {
    return (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 0xF);   // hwreg(HW_REG_XCC_ID, 0, 4)
}

// XCD agreement of a ring: every member publishes its XCC id and reads the ring's ids; the ring uses plain stores (the lines stay
// in that XCD's L2, the sc1 polls are L2 hits) iff all members sit on one XCD. A timeout is not an error: the write-through
// policy is valid for any placement. Every member reads the same published ids, so the choice is identical across the ring.
// Args: LstmArgs or LstmQ8Args (xcc_ws, max_spins, force_slow).
template <class Args>
__device__ __forceinline__ bool ring_store_policy(const Args& p, int ring, int slice, int nsl, int lane) {
    int* slot = p.xcc_ws + (long)ring * nsl;
    const int mine = xcc_id();
    if (lane == 0) __hip_atomic_store(slot + slice, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    bool ok = false;
    while (true) {
        bool any_unset = false, any_other = false;
        for (int i = lane; i < nsl; i += 64) {
            const int v = __hip_atomic_load(slot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            any_unset |= v < 0;
            any_other |= v != mine;
        }
        if (!__any(any_unset)) { ok = !__any(any_other); break; }
        if (++spins > p.max_spins) break;
        __builtin_amdgcn_s_sleep(4);
    }
    return ok && !p.force_slow;
}

// ---- 2. the bounded re-poll -----------------------------------------------------------------------------------------------------------
// A wave owns K pieces of what it waits for; `armed(kk)` is the wave-uniform test "piece kk still holds a sentinel" on the copy the wave
// has, `reload(kk)` fetches piece kk again (sc1: past the L1). The first round is the caller's (it is issued long before it is looked
// at); ring_pending tests it, ring_repoll re-fetches only what is still armed. Every spin is bounded: after max_spins rounds the wave
// raises *err once, goes on with what it has and never waits again (`dead`), so a lost partner ends the layer with an error instead of
// hanging the device. "lstm_tune" bit 0: spin without s_sleep. -> rounds, the first one included.
// The contract of a round: every reload(kk) of the pieces still pending is issued first, then armed(kk) is called EXACTLY ONCE per pending
// piece, in piece order. A caller whose reload lands somewhere else than in the copy it tests (wgx2: LDS-DMA) may therefore give
// ring_repoll an `armed` that first waits for the round's reloads and fetches the piece, then tests it; ring_pending's is a pure test.
template <int K, class Armed>
__device__ __forceinline__ unsigned ring_pending(Armed armed) {
    unsigned pend = 0;
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
        if (armed(kk)) pend |= (1u << kk);
    return pend;
}
template <int K, class Args, class Armed, class Reload>
__device__ __forceinline__ unsigned ring_repoll(const Args& p, int lane, bool& dead, unsigned pend, Armed armed, Reload reload) {
    unsigned spins = dead ? p.max_spins : 0u;   // after one timeout never wait again
    unsigned rounds = 1;
    while (pend != 0) {
        if (++spins > p.max_spins) {
            if (lane == 0 && !dead) atomicExch(p.err, 1);
            dead = true;
            break;
        }
        if (!(p.tune & 1)) __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
            if (pend & (1u << kk)) reload(kk);
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
            if ((pend & (1u << kk)) && !armed(kk)) pend &= ~(1u << kk);
        ++rounds;
    }
    return rounds;
}

// ---- 3. publish and re-arm ------------------------------------------------------------------------------------------------------------
// Vector stores with SCALAR addressing (a wave-uniform 64-bit base in an SGPR pair + a loop-invariant 32-bit per-lane byte offset)
template <bool SC1>
__device__ __forceinline__ void store8_s(const char* sbase, unsigned voff, unsigned long long v) {
    if constexpr (SC1) asm volatile("global_store_dwordx2 %0, %1, %2 sc1" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
    else asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
// One store under the ring's policy: plain (stays in this XCD's L2) or sc1 write-through (valid for any placement)
template <class W>
__device__ __forceinline__ void ring_store(W* dst, W v, bool fast) {
    if (fast) *dst = v;
    else __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The hand-off through the ring buffer: four time slots per ring ([4][R][tile], `exr` = this ring's tile in slot 0), h_t goes into slot
// step & 3 in fragment order (`my_byte`: this lane's four units, frag_byte below) as one word W (8 bytes fp16, 4 bytes int8), armed
// bytes read as ARM.
// The protocol: a consumer polls the data itself until no sentinel is left - no flags, no fences, no atomics, and every element is
// checked individually, so nothing depends on store granularity, dispatch order or workgroup -> XCD placement. A producer re-arms ITS
// OWN bytes of slot (step + 2) & 3 at step t. That slot holds h_{t-2}; the store sits behind the workgroup barrier of step t, which
// proves that the workgroup has seen every k-step of h_{t-1}, i.e. that EVERY wave of the ring has published h_{t-1} and hence finished
// reading h_{t-2} (a wave publishes only behind its workgroup's barrier, which follows all four quarter polls). The data store into the
// re-armed slot follows two steps later; the producer's vmcnt(0) ahead of its next barrier completes the re-arm before it publishes
// h_{t+1}, and nobody polls the slot for h_{t+2} before having seen everybody's h_{t+1}: no consumer can find stale bytes.
// `rearm` is the caller's statement: step >= 2 && step + 2 < T where the store count may vary (before step 2 the slots are still armed, in
// the last two steps nobody reads them any more), true where the operation count behind a poll round must be a constant (wgx2).
// SADDR: the scalar-addressed form of the stores (8-byte words only).
template <class W, W ARM, bool SADDR = false>
__device__ __forceinline__ void ring_publish(char* exr, long slot_stride, int step, int my_byte, W packed, bool fast, bool rearm) {
    char* cur = exr + (long)(step & 3) * slot_stride;
    char* nxt = exr + (long)((step + 2) & 3) * slot_stride;
    if constexpr (SADDR) {
        if (fast) store8_s<false>(cur, (unsigned)my_byte, packed); else store8_s<true>(cur, (unsigned)my_byte, packed);
        if (rearm) {
            if (fast) store8_s<false>(nxt, (unsigned)my_byte, ARM); else store8_s<true>(nxt, (unsigned)my_byte, ARM);
        }
    } else {
        ring_store((W*)(cur + my_byte), packed, fast);
        if (rearm) ring_store((W*)(nxt + my_byte), ARM, fast);
    }
}

// ---- 4. slice setup -------------------------------------------------------------------------------------------------------------------
// Workgroup -> (ring, first slice): block b sits on XCD b % 8 (speed only), the wpr workgroups of a ring are consecutive there.
// "lstm_tune" bit 5 (test hook): spread the workgroups of every ring over all eight XCDs, so that the placement-independent
// (write-through) hand-off really crosses XCDs.
struct RingSlice { int ring, slice; };
__device__ __forceinline__ RingSlice ring_slice(int wpr, int wave, int tune) {
    const int xcd = blockIdx.x & 7;
    const int lwg = blockIdx.x >> 3;
    const int rl = lwg / wpr;
    return {rl * 8 + ((tune & 32) ? ((xcd + (lwg - rl * wpr)) & 7) : xcd), (lwg - rl * wpr) * 4 + wave};
}
// The packed A fragments of a slice ([slice][m][k-step][lane][16 bytes], bh_lstm_pack / bh_k_lstm_q8_pack) -> registers
template <int MT, int NKS, class V, class E>
__device__ __forceinline__ void slice_frags(V (&w)[MT][NKS], const E* packed, int slice, int lane) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            w[m][ks] = *(const V*)(packed + ((((long)slice * MT + m) * NKS + ks) * 64 + lane) * (long)(sizeof(V) / sizeof(E)));
}
template <int MT, int NKS, class V, class E>
__device__ __forceinline__ void slice_frags(V (&whh)[MT][NKS], V (&wih)[MT][NKS], const E* whh_p, const E* wih_p, int slice, int lane) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const long o = ((((long)slice * MT + m) * NKS + ks) * 64 + lane) * (long)(sizeof(V) / sizeof(E));
            whh[m][ks] = *(const V*)(whh_p + o);
            wih[m][ks] = *(const V*)(wih_p + o);
        }
}
// Per-row constants ([4H], torch gate-major) of this lane's MT units u0 .. u0 + MT - 1: accumulator element i of tile m is gate i of unit u0 + m
template <int MT>
__device__ __forceinline__ void slice_rows(float4_t (&v)[MT], const float* rows, int H, int u0) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[m][i] = rows[i * H + u0 + m];
}
// The lanes that move a wave's U units out: lane -> (chunk cc, 4 consecutive units `part`)
struct RingMover { bool mover; int cc, part; };
template <int U>
__device__ __forceinline__ RingMover ring_mover(int lane) {
    constexpr int PARTS = U / 4;
    const int cc = lane / PARTS;
    return {lane < 16 * PARTS, cc, lane - cc * PARTS};
}
// THE fragment order: byte offset of unit u of chunk c inside a ring tile. EB = bytes per element (2: fp16, a k-step is 32 units;
// 1: int8, 64 units); lane (c, q) of a k-step holds 16 / EB consecutive units of chunk c.
template <int EB>
__device__ __forceinline__ int frag_byte(int u, int c) {
    constexpr int S = EB == 2 ? 3 : 4;
    return (((u >> (S + 2)) * 64 + ((u >> S) & 3) * 16 + c) << 4) + (u & ((1 << S) - 1)) * EB;
}

// ---- 5. LDS-DMA -----------------------------------------------------------------------------------------------------------------------
// One 1 KiB global -> LDS DMA: lane l moves 16 bytes from g (per lane) to lds + 16 l (lds is wave-uniform), which IS the fragment order.
// The compiler neither counts nor waits for it: the issuing wave covers it with its own s_waitcnt vmcnt ahead of the barrier that
// publishes it. POLL: sc0 sc1, a poll of the exchange (past the L1 and this XCD's L2 policy).
template <bool POLL>
__device__ __forceinline__ void dma16(const char* g, char* lds) {
    const unsigned l = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(__attribute__((address_space(3))) char*)lds);
    if constexpr (POLL) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off sc0 sc1" ::"s"(l), "v"(g) : "memory");
    else asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(l), "v"(g) : "memory");
}
// The same with SCALAR addressing (the H = 384 fast paths): a wave-uniform 64-bit base in an SGPR pair plus a 32-bit per-lane byte
// offset that is loop-invariant (the compiler's per-lane 64-bit address arithmetic, the generic -> LDS pointer conversions in front
// of every M0 write and the spilled scalars behind them were ~55 instructions for the three x-stream DMAs of a ring step alone).
// IMM: immediate byte offset (13-bit signed) - keep it 0 for LDS-DMA: the hardware adds the instruction offset to the LDS address as
// well as to the global one. The DMA lands at LDS address lds_a + lane * 16.
template <int IMM, bool POLL>
__device__ __forceinline__ void dma16_s(const char* sbase, unsigned voff, unsigned lds_a) {
    if constexpr (POLL)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%3 sc0 sc1" ::"s"(lds_a), "v"(voff), "s"(sbase), "i"(IMM) : "memory");
    else
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%3" ::"s"(lds_a), "v"(voff), "s"(sbase), "i"(IMM) : "memory");
}

// ---- 6. input projection and x stream -------------------------------------------------------------------------------------------------
// The x stream never touches registers: wave w moves k-steps 3 - w, 7 - w, .. of a tile (balanced against its polls w, w + 4, ..) from
// `src` (this lane's 16 bytes of k-step 0; a k-step further is `ks_bytes` further) into tile `slot` of the LDS tiles at `xbuf`. (The LDS
// address is one sum on purpose: with the tile's address formed first, hipcc's backend stops at an illegal instruction in wgx2.)
template <int NKS>
__device__ __forceinline__ void x_dma(const char* src, int ks_bytes, char* xbuf, int slot, int wave) {
#pragma unroll
    for (int kk = 0; kk < (NKS + 3) / 4; ++kk) {
        const int ks = (3 - wave) + 4 * kk;
        if (NKS % 4 == 0 || ks < NKS) dma16<false>(src + ks * ks_bytes, xbuf + (slot * NKS + ks) * 1024);
    }
}

// MFMA whose A operand (a stationary fragment) lives in the accumulation-register half of the unified register file, accumulator in
// VGPRs; _vv: everything in VGPRs. The compiler does not track MFMA hazards through inline asm: callers keep >= 19 wait states between the
// last of them and the first VALU read of `c` (mfma_settle_v) and never issue one directly after a VALU write of its operands.
__device__ __forceinline__ void mfma16_av(const half8_t& a_agpr, const half8_t& b, float4_t& c) {
    asm("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "a"(a_agpr), "v"(b));
}
__device__ __forceinline__ void mfma16_vv(const half8_t& a, const half8_t& b, float4_t& c) {
    asm("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
template <int MT>
__device__ __forceinline__ void mfma_settle_v(float4_t (&c)[MT]) {
    if constexpr (MT == 3) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]));
    else asm volatile("s_nop 15\n\ts_nop 7" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
}
// Input projection of one step from the LDS tile xb (fragment reads one k-step ahead of their MFMAs): xa = bias + W_ih x_t
template <int NKS, int MT>
__device__ __forceinline__ void x_phase(float4_t (&xa)[MT], const float4_t (&bias4)[MT], const half8_t (&wih)[MT][NKS], const char* xb, int lo) {
#pragma unroll
    for (int m = 0; m < MT; ++m) xa[m] = bias4[m];
    half8_t b_cur = *(const half8_t*)(xb + lo), b_nxt = b_cur;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (ks + 1 < NKS) b_nxt = *(const half8_t*)(xb + (ks + 1) * 1024 + lo);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < MT - 1) mfma16_av(wih[m][ks], b_cur, xa[m]);
            else mfma16_vv(wih[m][ks], b_cur, xa[m]);
        }
        b_cur = b_nxt;
    }
    mfma_settle_v<MT>(xa);
}

// ---- 7. statistics ("lstm_tune" bit 2) --------------------------------------------------------------------------------------------------
// The workspace: XCD agreement slots [n_rings][nsl] int, a gap, then WORDS int64 per wave (bh_k_lstm_ws_bytes sizes it for the most
// waves and words any kernel has). What a kernel stamps into its words is read by tools/lstm_stats2.py, lstm_wide_stats.py, lstm_q8_stats.py.
constexpr size_t LSTM_STATS_GAP = 64;
constexpr int LSTM_STATS_WORDS = 16;
template <int WORDS = LSTM_STATS_WORDS>
__device__ __forceinline__ long long* lstm_stats_slot(int* xcc_ws, int n_rings, int nsl, int ring, int slice) {
    static_assert(WORDS <= LSTM_STATS_WORDS, "bh_k_lstm_ws_bytes");
    return (long long*)((char*)xcc_ws + (((size_t)n_rings * nsl * sizeof(int) + LSTM_STATS_GAP + 7) & ~(size_t)7)) + ((long)ring * nsl + slice) * WORDS;
}

}  // namespace bh
