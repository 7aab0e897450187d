// rs16_pass_launch.hip -- launch_pass: which pass kernel a launch takes and
// how it is launched.  The kernels themselves are instantiated in
// rs16_pass_enc.hip, rs16_pass_dec.hip, rs16_pass_tower.hip, rs16_pass_repair.hip,
// rs16_pass_select.hip and rs16_pass_verify.hip (template:
// rs16_pass.hpp); this unit sees them through the PassKernel lookups only.
#include <algorithm>

#include "rs16_pass_common.hpp"

namespace rs16 {

// The kernel of (prog, T, nv) (fn nullptr: no such variant): one table,
// filled at the first launch from whichever unit instantiates the program.
struct KernelTable {
    PassKernel k[NUM_PROGS][9][NARROW_VARIANTS];
    KernelTable() {
        for (int prog = 0; prog < NUM_PROGS; prog++)
            for (int T = 0; T <= 8; T++)
                for (int nv = 0; nv < NARROW_VARIANTS; nv++) {
                    PassKernel& e = k[prog][T][nv];
                    e = pass_kernels_enc(prog, T, nv);
                    if (!e.fn) e = pass_kernels_dec(prog, T, nv);
                    e.late[Z_PAIRED] = pass_kernels_paired(prog, T, nv);
                    e.late[Z_TOWER] = pass_kernels_tower(prog, T, nv);
                    e.wide3 = nv == 0 ? pass_kernel_tower_wide3(prog, T) : nullptr;
                }
    }
};
// The repair's programs (ids behind the profiling ids; rs16_pass_repair.hip):
// one kernel per (prog, T), no narrow variants, no late-rows flavours.
struct RepairTable {
    PassKernel k[2][9], none{};
    RepairTable() {
        static_assert(DEC_SINGLE_ALL == DEC_LAST_ALL + 1, "the table's rows");
        for (int p = 0; p < 2; p++)
            for (int T = 0; T <= 8; T++) k[p][T] = pass_kernels_repair(DEC_LAST_ALL + p, T);
    }
};
// The selective decode's programs (rs16_pass_select.hip), likewise.
struct SelectTable {
    PassKernel k[2][9], none{};
    SelectTable() {
        static_assert(DEC_SINGLE_SEL == DEC_LAST_SEL + 1, "the table's rows");
        for (int p = 0; p < 2; p++)
            for (int T = 0; T <= 8; T++) k[p][T] = pass_kernels_select(DEC_LAST_SEL + p, T);
    }
};
// The scrub's programs (rs16_pass_verify.hip), likewise.
struct VerifyTable {
    PassKernel k[2][9], none{};
    VerifyTable() {
        static_assert(ENC_SINGLE_VFY == ENC_LAST_VFY + 1, "the table's rows");
        for (int p = 0; p < 2; p++)
            for (int T = 0; T <= 8; T++) k[p][T] = pass_kernels_verify(ENC_LAST_VFY + p, T);
    }
};
static const PassKernel& find_kernel(int prog, int T, int nv) {
    if (repair_prog(prog)) {
        static const RepairTable repair;
        return nv == 0 ? repair.k[prog - DEC_LAST_ALL][T] : repair.none;
    }
    if (select_prog(prog)) {
        static const SelectTable select;
        return nv == 0 ? select.k[prog - DEC_LAST_SEL][T] : select.none;
    }
    if (verify_prog(prog)) {
        static const VerifyTable verify;
        return nv == 0 ? verify.k[prog - ENC_LAST_VFY][T] : verify.none;
    }
    static const KernelTable table;
    return table.k[prog][T][nv];
}

// The kernel of a launch: among the variants that exist for (prog, T), the
// one that uses the narrow multiply in the most layers the launch allows
// (ni / nf: first_narrow_layer of its IFFT / FFT direction).
static int pick_variant(int prog, int T, int ni, int nf) {
    for (int nv = 1; nv < NARROW_VARIANTS; nv++) {
        const int vi = nv == 2 ? 1 : 0, vf = nv == 3 ? 1 : 0;  // NarrowVar<nv>::IFFT_FROM / FFT_FROM
        if (ni > vi || nf > vf) continue;
        if (find_kernel(prog, T, nv).fn) return nv;
    }
    return 0;
}

const PassKernel& pass_kernel_of(int prog, int T) { return find_kernel(prog, T, 0); }

PassConsts pass_launch_consts(const PassKernel& k, int T, const PassArgs& a) {
    PassConsts c;
    c.nslab = (a.qrow + k.quads - 1) / k.quads;
    {
        const uint64_t hws = k.quads >= 64 ? 1 : 64 / k.quads;
        // (vfy_S: the stored rows the scrub's programs compare with, 0 in every other launch)
        const uint64_t smax = std::max(std::max(std::max(a.S_in, a.S_out), std::max(a.S_seg, a.S_rest)), a.vfy_S);
        const uint64_t span = (uint64_t)1 << (T + a.lo);  // rows of one tile's aligned block
        // A lane's byte offset below its wave's row base is lane_rows x S +
        // offL (rs16_pass.hpp LaneOff): lane_rows, the rows from the wave's
        // first row set to the lane's, at most (hws - 1) 2^R << lo in layout A
        // (2^R <= 16 rows per row set; layout B: (hws - 1) << lo), S any of
        // the four strides, offL the lane's quad within the slice, whose high
        // dword ends at 8 qrow: the last byte a lane touches lies at most at
        // (hws - 1) (16 << lo) smax + 8 qrow - 1, which has to stay below 2^32.
        // (With one row set per wave, T = 7 and T <= 4, the offset is offL
        // alone.  A lane without a quad forms a larger offset and uses none.)
        const bool fits = (hws - 1) * ((uint64_t)16 << a.lo) * smax + 8 * (uint64_t)a.qrow <= ((uint64_t)1 << 32);
        const bool aligned = a.chunk % span == 0 && a.row_base_in % span == 0;
        // (RS16_DIAG_FORCE_VOFF64: always the 64-bit lane offsets)
        c.voff32 = fits && aligned && !(a.diag & DIAG_FORCE_VOFF64) ? 1u : 0u;
    }
    // The full-item fast path's launch constants (PassArgs::rs_in).
    c.rs_in = a.S_in << (a.lo + k.load_shb);
    c.rs_seg = a.S_seg << (a.lo + k.load_shb);
    c.rs_out = a.S_out << (a.lo + k.store_shb);
    // (16 row registers at most: the stores' offsets m x rs_out fit 32 bits)
    const bool full = c.voff32 && a.qrow % k.quads == 0 && a.in_rows_mask == 0 && c.rs_out < ((uint64_t)1 << 28);
    c.full_lanes = full ? 1u : 0u;
    // The late-rows variant (pass_kernel_late) has no general row loads: it
    // runs exactly when every wave of the launch is ROWS_DIRECT or ROWS_ZERO
    // (wave_rows_mode) -- 32-bit lane offsets, no row mask, and, in the
    // gathering first pass, a row limit that cuts through no wave's rows.  A
    // wave of that pass (layout A) holds the rows base + (k << lo), k < hws
    // 2^R, with base = b_low + j (hws 2^R << lo) over all b_low < 2^lo and all
    // j: a_count = j0 (hws 2^R << lo) + r lies strictly inside the range of
    // wave (b_low, j0) when b_low < r <= b_low + ((hws 2^R - 1) << lo), which
    // some b_low satisfies for every r != 0 and none for r = 0.  So: a_count a
    // multiple of hws 2^R << lo.  Partial slabs and waves wholly above the
    // limit (the zero page) qualify.  Its row registers are addressed as base
    // + m x stride in 32 bits (m <= 15): the strides stay below 2^28.
    // (RS16_DIAG_NO_LATE_ROWS: never.)
    {
        const uint64_t hws = k.quads >= 64 ? 1 : 64 / k.quads;
        const uint64_t wave_span = (hws << k.reg_bits) << a.lo;
        const bool whole = !k.gather || a.a_count % wave_span == 0;
        const bool strides = c.rs_in < ((uint64_t)1 << 28) && c.rs_seg < ((uint64_t)1 << 28);
        const bool on = k.late[Z_SHARD] && !(a.diag & DIAG_NO_LATE_ROWS);
        c.late_rows = on && c.voff32 && a.in_rows_mask == 0 && whole && strides ? 1u : 0u;
    }
    return c;
}

// The three launches of a sequence (encode_high_fused, the identity branch of
// decode_passes): lo contiguous row bits (row_split) gathered from the caller's
// rows (stride S_user), hi strided ones on the work buffer, lo contiguous ones
// stored to the caller's rows.  Tower form goes with the paired form: the same
// gate, its own switch, and a tower flavour of each of the three kernels.
ZForm z_form_sequence(uint32_t chunk_rows, uint64_t S, uint64_t S_user, uint32_t a_count, uint32_t seg_chunk,
                      uint32_t row_base_in, int diag) {
    if (diag & DIAG_NO_PAIRED_ROWS) return Z_SHARD;
    if (chunk_rows < 512 || (chunk_rows & (chunk_rows - 1)) || S == 0 || S % 8 || S / 8 > 0xFFFFFFFFu) return Z_SHARD;
    const RowSplit sp = row_split(__builtin_ctz(chunk_rows));  // (a power of two)
    PassArgs a{};
    a.S_in = a.S_out = a.S_rest = S;
    a.S_seg = S_user;
    a.qrow = (uint32_t)(S / 8);
    a.a_count = a_count, a.chunk = seg_chunk, a.row_base_in = row_base_in;
    a.diag = (uint32_t)diag;
    const struct { int prog, T; uint32_t lo; uint64_t S_out; } seq[3] = {
        {ENC_FIRST, sp.lo, 0, S}, {ENC_MID, sp.hi, (uint32_t)sp.lo, S}, {ENC_LAST, sp.lo, 0, S_user}};
    bool tower = !(diag & DIAG_NO_TOWER_ROWS);
    for (const auto& p : seq) {
        if (p.T > 8) return Z_SHARD;
        // (the geometry and the flavours of (prog, T) are those of every narrow variant)
        const PassKernel& k = find_kernel(p.prog, p.T, 0);
        a.lo = p.lo, a.S_out = p.S_out;
        const PassConsts c = pass_launch_consts(k, p.T, a);
        if (!k.fn || !k.late[Z_PAIRED] || !c.late_rows || !c.full_lanes) return Z_SHARD;
        tower = tower && k.late[Z_TOWER];
    }
    return tower ? Z_TOWER : Z_PAIRED;
}

hipError_t launch_pass(int prog, int T, const PassArgs& args, uint32_t num_tiles, hipStream_t s) {
    const bool appended = repair_prog(prog) || select_prog(prog) || verify_prog(prog);  // (the programs behind the profiling ids)
    if (prog < 0 || (prog >= NUM_PROGS && !appended) || T < 0 || T > 8) return hipErrorInvalidValue;
    if (appended && !find_kernel(prog, T, 0).fn) return hipErrorInvalidValue;  // (*_LAST_*: T >= 4, *_SINGLE_*: T >= 1)
    if (select_prog(prog) && !args.wanted) return hipErrorInvalidValue;  // (the read set is dereferenced)
    // (the stored rows and the row flags are dereferenced)
    if (verify_prog(prog) && (!args.vfy_cmp || !args.vfy_rows)) return hipErrorInvalidValue;
    if (num_tiles == 0 || args.qrow == 0) return hipSuccess;
    PassArgs a = args;
    // Narrow twiddles: the launch's tiles are tile_base + [0, tiles of one
    // stripe), b_high = tile >> lo (RS16_DIAG_WIDE_TWIDDLES: never)
    int ni = T, nf = T;
    const uint32_t bh_max = (a.tile_base + (a.stripe_tiles ? a.stripe_tiles : num_tiles) - 1) >> a.lo;
    if (!(a.diag & DIAG_WIDE_TWIDDLES)) {
        ni = first_narrow_layer(a.lo, T, a.skew_ifft, bh_max);
        nf = first_narrow_layer(a.lo, T, a.skew_fft, bh_max);
    }
    int nv = pick_variant(prog, T, ni, nf);
    // The tower middle pass of variant 2 / 3 multiplies in its one wide layer
    // (layer 0 of the IFFT / FFT) by twiddles s ^ v_8, s in the subfield
    // (mul_xor_tower_beta): a launch whose layer has any other twiddle takes
    // the 12-lookup kernel.
    if (a.z_form == Z_TOWER && ((nv == 2 && !layer_beta(a.lo, 0, T, a.skew_ifft, bh_max)) ||
                                (nv == 3 && !layer_beta(a.lo, 0, T, a.skew_fft, bh_max))))
        nv = 0;
    const PassKernel& k = find_kernel(prog, T, nv);
    const PassConsts pc = pass_launch_consts(k, T, a);
    a.nslab = pc.nslab;
    a.ntiles = num_tiles;
    const uint32_t nwg = num_tiles * a.nslab;  // one workgroup per (tile, slab) item
    if (a.need_hi == 0) a.need_hi = 1u << T;  // no pruning
    a.voff32 = pc.voff32;
    a.fd_lds = (a.diag & DIAG_FD_LDS) ? 1u : 0u;
    a.rs_in = pc.rs_in, a.rs_seg = pc.rs_seg, a.rs_out = pc.rs_out;
    a.full_lanes = pc.full_lanes;
    const FastDiv dn = fast_div_of(a.nslab), ds = fast_div_of(a.stripe_tiles);
    a.nslab_mul = dn.mul, a.nslab_one = dn.one;
    a.stripe_mul = ds.mul, a.stripe_one = ds.one;
    const size_t lds = (size_t)k.lds;
    PassFn fn = pc.late_rows ? k.late[Z_SHARD] : k.fn;
    if (a.z_form != Z_SHARD) {
        // The form is the sequence's choice (z_form_sequence): a launch that
        // cannot keep it is an error, never another form -- its neighbour
        // pass would read or write the rows the other way.
        const bool in_sequence = prog == ENC_FIRST || prog == ENC_MID || prog == ENC_LAST;
        if (a.z_form > Z_TOWER || !in_sequence || !pc.late_rows || !pc.full_lanes || !k.late[a.z_form])
            return hipErrorInvalidValue;
        fn = k.late[a.z_form];
        // The first and last pass of a tower sequence multiply by three byte
        // maps, in every layer and for every twiddle: the same kernel but for
        // the multiply (RS16_DIAG_WIDE_TWIDDLES: the 12 lookups of late[]).
        if (a.z_form == Z_TOWER && k.wide3 && !(a.diag & DIAG_WIDE_TWIDDLES)) fn = k.wide3;
    }
    if (lds > 65536) {
        // (per kernel variant: each is a function of its own)
        hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 grid(nwg), block(k.threads);
    hipLaunchKernelGGL(fn, grid, block, lds, s, a);
    return hipGetLastError();
}

}  // namespace rs16
