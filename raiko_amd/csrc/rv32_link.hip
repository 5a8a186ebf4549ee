// The link between shard memories read off a finished memory table (include/raiko_hip.h: rk_rv32mem_journal_device and
// its host twin rk_rv32mem_journal_root; raiko_amd/rv32link.py): one kernel, its driver and the host's Merkle root.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "rv32_tiles.hpp"

namespace rv32 {

// One lane per row of the memory table.  The block's rows come in as whole lines through LDS (stride 13: odd); a lane decodes its row's six limbs and REAL, writes
// the link row (the six limbs as they are, Montgomery; zeros on a padding row) and the journal row (word address, INIT,
// FINAL, canonical; zeros likewise) into LDS, and both tiles leave as whole lines.  A block's count of real rows is one
// __syncthreads_count.  err |= ERR_JOURNAL: REAL is not boolean, a real row follows a padding row (lane 0 of a later block reads
// the row before its tile from HBM), or a limb of a real row is no 16-bit (WL: 14-bit) value.
static_assert(B_WL == 0 && B_F_HI + 1 == RK_RV32LINK_TUPLE, "the link tuple is the memory row's first six cells");
__global__ void __launch_bounds__(TB) mem_journal_kernel(const uint32_t* __restrict__ mem, uint32_t* __restrict__ journal,
                                                          uint32_t* __restrict__ link, uint32_t* __restrict__ count,
                                                          uint32_t* __restrict__ err) {
    constexpr unsigned LW = RK_RV32LINK_TUPLE, LS = LW | 1, JW = 3;
    __shared__ uint32_t s_in[TB * BD_W], s_link[TB * LS], s_j[TB * JW];
    const unsigned nb = blockDim.x;
    const size_t r0 = (size_t)blockIdx.x * nb;
    for (unsigned k = threadIdx.x; k < nb * BD_W; k += nb) s_in[k] = mem[r0 * BD_W + k];
    __syncthreads();
    const uint32_t* row = s_in + threadIdx.x * BD_W;
    const uint32_t real = bb::decode(row[B_REAL]);
    const uint32_t prev = threadIdx.x ? bb::decode(s_in[(threadIdx.x - 1) * BD_W + B_REAL])
                                      : (r0 ? bb::decode(mem[(r0 - 1) * BD_W + B_REAL]) : 1u);
    uint32_t c[LW];
    uint32_t over = 0;
#pragma unroll
    for (unsigned j = 0; j < LW; j++) {
        c[j] = bb::decode(row[B_WL + j]);
        over |= c[j] >> 16;
    }
    over |= c[B_WL] >> 14;
    const bool on = real == 1;
    if (real > 1 || (on && (prev != 1 || over))) atomicOr(err, ERR_JOURNAL);
#pragma unroll
    for (unsigned j = 0; j < LW; j++) s_link[threadIdx.x * LS + j] = on ? row[B_WL + j] : 0u;
    s_j[threadIdx.x * JW + 0] = on ? (c[B_WL] | c[B_WH] << 14) : 0u;
    s_j[threadIdx.x * JW + 1] = on ? (c[B_I_LO] | c[B_I_HI] << 16) : 0u;
    s_j[threadIdx.x * JW + 2] = on ? (c[B_F_LO] | c[B_F_HI] << 16) : 0u;
    const int n_real = __syncthreads_count(on);
    if (threadIdx.x == 0 && n_real) atomicAdd(count, (uint32_t)n_real);
    for (unsigned k = threadIdx.x; k < nb * LW; k += nb) link[r0 * LW + k] = s_link[(k / LW) * LS + k % LW];
    for (unsigned k = threadIdx.x; k < nb * JW; k += nb) journal[r0 * JW + k] = s_j[k];
}

// rk_rv32mem_journal_device: the kernel, then the library's own commitment of the link matrix.  The two scratch words
// (count, error) are read back after the tree is built; the stream is drained before they go
static int journal_device(rk_ctx* ctx, const uint32_t* d_memory, size_t memory_rows, uint32_t* d_journal, uint32_t* d_link,
                          uint32_t* d_nodes, size_t* n_real, uint32_t h_root[8]) {
    if (!ctx || !d_memory || !d_journal || !d_link || !d_nodes || !n_real || !h_root) return RK_ERR_INVALID;
    if (memory_rows < 2 || (memory_rows & (memory_rows - 1)) || memory_rows > ((size_t)1 << ntt::LAMBDA)) return RK_ERR_INVALID;
    *n_real = 0;
    RK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* d_flags = nullptr;
    RK_TRY(rk::dev_alloc(ctx, 8, &d_flags));
    uint32_t flags[2] = {0, 0};
    auto enqueue = [&]() -> int {
        RK_HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, 8, ctx->stream));
        const unsigned b = (unsigned)std::min<size_t>(memory_rows, TB);
        RK_TRY(rk::launch(ctx, "rv32 mem_journal_kernel", mem_journal_kernel, (unsigned)(memory_rows / b), b, 0, d_memory, d_journal,
                          d_link, (uint32_t*)d_flags, (uint32_t*)d_flags + 1));
        const rk_matrix m{d_link, (uint32_t)memory_rows, RK_RV32LINK_TUPLE, 1};
        RK_TRY(rk_mmcs_commit(ctx, &m, 1, d_nodes, h_root));
        return rk::d2h_sync(ctx, flags, d_flags, 8);
    };
    int st = enqueue();
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess && st == RK_OK) {
        ctx->last_error = std::string("rk_rv32mem_journal_device sync: ") + hipGetErrorString(e);
        st = RK_ERR_HIP;
    }
    rk::dev_free(ctx, d_flags);
    if (st != RK_OK) return st;
    if (flags[1]) {
        ctx->last_error = "rk_rv32mem_journal_device: the memory table's real rows are not a prefix or a limb is out of range";
        return RK_ERR_INVALID;
    }
    *n_real = flags[0];
    return RK_OK;
}

// the digest of a journal on the host: the leaves of the real rows, then level by level the nodes above a real row; a
// subtree of zero rows has one digest per level.  Linear in the journal's rows (n log_rows compressions at most)
static int journal_root(const rk_params* params, const uint32_t* journal, size_t n, uint32_t log_rows, uint32_t root[8]) {
    if (!root || (n && !journal) || log_rows < 1 || log_rows > ntt::LAMBDA || n > ((size_t)1 << log_rows)) return RK_ERR_INVALID;
    for (size_t i = 0; i < n; i++)
        if (journal[3 * i] >= (1u << 30) || (i && journal[3 * i] <= journal[3 * (i - 1)])) return RK_ERR_INVALID;
    rk_params def;
    rk::params_preset(&def, RK_PRESET_SP1);
    rk::Sys sys;
    auto k = std::make_unique<p2::Any>();
    RK_TRY(rk::resolve_params(params ? params : &def, &sys, k.get()));
    uint32_t zero[8], row[RK_RV32LINK_TUPLE] = {0};
    k->hash_elems(row, RK_RV32LINK_TUPLE, zero);
    std::vector<uint32_t> cur(8 * std::max<size_t>(n, 1));
    for (size_t i = 0; i < n; i++) {
        const uint32_t a = journal[3 * i], init = journal[3 * i + 1], fin = journal[3 * i + 2];
        const uint32_t limbs[RK_RV32LINK_TUPLE] = {a & 0x3fffu, a >> 14, init & 0xffffu, init >> 16, fin & 0xffffu, fin >> 16};
        for (unsigned j = 0; j < RK_RV32LINK_TUPLE; j++) row[j] = enc(limbs[j]);
        k->hash_elems(row, RK_RV32LINK_TUPLE, &cur[8 * i]);
    }
    size_t cnt = n;
    for (uint32_t lvl = 0; lvl < log_rows; lvl++) {
        const size_t up = (cnt + 1) / 2;
        for (size_t i = 0; i < up; i++) {
            uint32_t out[8];
            k->hash_pair(&cur[16 * i], 2 * i + 1 < cnt ? &cur[16 * i + 8] : zero, out);
            std::memcpy(&cur[8 * i], out, 32);
        }
        uint32_t z2[8];
        k->hash_pair(zero, zero, z2);
        std::memcpy(zero, z2, 32);
        cnt = up;
    }
    std::memcpy(root, cnt ? cur.data() : zero, 32);
    return RK_OK;
}

}  // namespace rv32

extern "C" {

int rk_rv32mem_journal_device(rk_ctx* ctx, const uint32_t* d_memory, size_t memory_rows, uint32_t* d_journal, uint32_t* d_link,
                              uint32_t* d_nodes, size_t* n_real, uint32_t h_root[8]) {
    RK_GUARD_BEGIN
    return rv32::journal_device(ctx, d_memory, memory_rows, d_journal, d_link, d_nodes, n_real, h_root);
    RK_GUARD_END
}
int rk_rv32mem_journal_root(const rk_params* params, const uint32_t* journal, size_t n, uint32_t log_rows, uint32_t root[8]) {
    RK_GUARD_BEGIN
    return rv32::journal_root(params, journal, n, log_rows, root);
    RK_GUARD_END
}

}  // extern "C"
