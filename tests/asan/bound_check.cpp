// CPU-only sanitizer harness (g++ -fsanitize=address,undefined): calls the HIP-free shape checks of
// the C ABI (raiko_amd/csrc/taps.hpp: rk::check_taps, rk::seal_bound_words -- what
// rk_seal_bound_words, rk_prove_segment and rk_verify_segment_ex run first) on malformed tap sets
// held in exactly-sized heap arrays, so any out-of-bounds read aborts; and the facts of a seal's
// shape that prover, verifier and bound share (taps per register, Merkle cap, FRI round walk), which
// may only be asked of a tap set check_taps accepted.
#include <cstdio>
#include <cstring>
#include <vector>

#include "taps.hpp"

struct Shape {
    std::vector<uint32_t> rg, ro, rc, off, backs;
    rk_segment seg;
    Shape(uint32_t wa, uint32_t wc, uint32_t wd) {
        std::memset(&seg, 0, sizeof seg);
        uint32_t gs[3] = {wa, wc, wd};
        for (uint32_t g = 0; g < 3; g++)
            for (uint32_t o = 0; o < gs[g]; o++) {
                rg.push_back(g);
                ro.push_back(o);
                rc.push_back(g == 0 ? 1 : 0);
            }
        off = {0, 1, 3};
        backs = {0, 0, 1};
        sync();
        seg.po2 = 10;
        for (int g = 0; g < 3; g++) seg.taps.group_size[g] = gs[g];
        seg.taps.n_combos = 2;
        seg.n_globals = 4;
    }
    void sync() {
        seg.taps.n_regs = (uint32_t)rg.size();
        seg.taps.reg_group = rg.data();
        seg.taps.reg_offset = ro.data();
        seg.taps.reg_combo = rc.data();
        seg.taps.combo_off = off.data();
        seg.taps.combo_backs = backs.data();
    }
};

static int fails = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what);
        fails++;
    }
}
// the contract of the shape helpers: check_taps first; they run only on what it accepted
static bool refused(const rk_taps& t) {
    if (rk::check_taps(t) != RK_OK) return true;
    size_t sum = 0;
    for (uint32_t r = 0; r < t.n_regs; r++) sum += rk::reg_taps(t, r);
    expect(sum == rk::total_taps(t) && rk::max_back(t) <= 64, "helpers on an accepted tap set");
    return false;
}
static size_t fri_rounds(size_t n, uint32_t fold_log2, uint32_t min_degree, size_t* final_degree) {
    rk::Shape sh;
    sh.fold_log2 = fold_log2;
    sh.min_degree = min_degree;
    size_t rounds = 0, last = 0;
    *final_degree = rk::fri_walk(n, sh, [&](size_t size, size_t domain) {
        expect(domain == size << sh.blowup_log2 && (rounds == 0 || size < last), "round sizes fall, domain = size << blow-up");
        last = size;
        rounds++;
    });
    return rounds;
}

int main() {
    {
        Shape s(4, 4, 8);
        expect(rk::check_taps(s.seg.taps) == RK_OK, "well-formed taps accepted");
        expect(rk::seal_bound_words(&s.seg) > 0, "bound of a well-formed shape");
        expect(!refused(s.seg.taps), "helpers run on the well-formed shape");
        expect(rk::total_taps(s.seg.taps) == 4 * 2 + 4 + 8 && rk::reg_taps(s.seg.taps, 0) == 2 && rk::reg_taps(s.seg.taps, 15) == 1,
               "taps per register and in total");
        expect(rk::combo_taps(s.seg.taps, 1) == 2 && rk::max_back(s.seg.taps) == 1, "taps of a combo, largest back");
    }
    {
        Shape s(4, 4, 8);
        s.rc[0] = 99;  // combo id far outside combo_off
        expect(rk::check_taps(s.seg.taps) == RK_ERR_INVALID, "combo id out of range");
        expect(rk::seal_bound_words(&s.seg) == 0, "bound is 0 for a bad combo id");
        expect(refused(s.seg.taps), "no helper runs on a bad combo id");
    }
    {
        Shape s(4, 4, 8);
        s.off = {0, 3, 1};  // not monotone: differences would underflow
        s.sync();
        expect(rk::seal_bound_words(&s.seg) == 0, "non-monotone combo_off");
        expect(refused(s.seg.taps), "no helper runs on a non-monotone combo_off");
    }
    {
        Shape s(4, 4, 8);
        s.ro[5] = 77;  // offset outside its group
        expect(rk::seal_bound_words(&s.seg) == 0, "register offset out of range");
        expect(refused(s.seg.taps), "no helper runs on a bad register offset");
    }
    {
        Shape s(4, 4, 8);
        s.seg.taps.group_size[2] = 9;  // sizes do not add up to n_regs
        expect(rk::seal_bound_words(&s.seg) == 0, "group sizes vs n_regs");
        expect(refused(s.seg.taps), "no helper runs when the group sizes do not add up");
    }
    {
        Shape s(4, 4, 8);
        s.backs = {0, 0, 200};
        s.sync();
        expect(rk::seal_bound_words(&s.seg) == 0, "back beyond the supported range");
        expect(refused(s.seg.taps), "no helper runs on a back beyond the range");
    }
    {
        Shape s(4, 4, 8);
        s.seg.taps.combo_off = nullptr;
        expect(rk::seal_bound_words(&s.seg) == 0, "null array");
        expect(refused(s.seg.taps), "no helper runs on a null array");
        s.sync();
        s.seg.po2 = 0;
        expect(rk::seal_bound_words(&s.seg) == 0, "po2 = 0");
        s.seg.po2 = 23;
        expect(rk::seal_bound_words(&s.seg) == 0, "po2 too large");
        expect(rk::seal_bound_words(nullptr) == 0, "null segment");
    }
    {
        // the Merkle cap: the largest layer below the leaves that is no wider than the query count
        expect(rk::merkle_top_layer(2, 50) == 0, "two rows: the root alone");
        expect(rk::merkle_top_layer(4, 50) == 1 && rk::merkle_top_layer(1 << 12, 50) == 5, "cap limited by height, then by queries");
        expect(rk::merkle_top_layer(1 << 12, 1) == 0 && rk::merkle_top_layer(2, 1) == 0, "one query: the root alone");
        expect(rk::merkle_top_layer(1 << 12, 64) == 6 && rk::merkle_top_layer(1 << 12, 63) == 5, "queries at a power of two");
        expect(rk::merkle_top_layer(1 << 6, RK_MAX_QUERIES) == 5, "never the leaves themselves");
        // the FRI round walk
        size_t fin = 0;
        expect(fri_rounds(256, 4, 256, &fin) == 0 && fin == 256, "a size equal to min_degree gives no round");
        expect(fri_rounds(8, 4, 1, &fin) == 0 && fin == 8, "a size below the fold arity gives no round");
        expect(fri_rounds(512, 4, 256, &fin) == 1 && fin == 32, "one round");
        expect(fri_rounds(1 << 13, 4, 256, &fin) == 2 && fin == 32, "two rounds");
        expect(fri_rounds(16, 4, 1, &fin) == 1 && fin == 1, "a size equal to the fold arity folds once");
        expect(fri_rounds(1 << 22, 1, 1, &fin) == 22 && fin == 1, "fold 2 down to a constant");
    }
    std::printf(fails ? "%d failures\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
