// rs16_api_locate.cpp -- C ABI (include/rs16.h): locating the one corrupt shard
// of each 64-byte column block of a stripe (rs16_locate_plan,
// rs16_locate_device / _batch) and fixing it in place (rs16_heal_device /
// _batch).
#include "rs16_api.hpp"

using namespace rs16;

// ---------------------------------------------------------------------------
// The encode is GF(2^16)-linear per element position, recovery_j = sum_i
// M[j][i] original_i, and the code is MDS.  With syndrome_j = encode(stored
// originals)_j ^ stored recovery_j, one corrupt recovery shard j leaves exactly
// syndrome_j nonzero, and one corrupt original i with error e makes every
// syndrome nonzero, syndrome_j = M[j][i] e; then syndrome_0 / syndrome_1 =
// M[0][i] / M[1][i] names i (every 2 x 2 minor of M is nonzero, so the k ratios
// differ) and e = syndrome_0 / M[0][i].  A plan holds rows 0 and 1 of M as logs.
// ---------------------------------------------------------------------------
struct rs16_locate_plan {
    rs16_engine* eng;  // nullptr once the engine was freed (detached)
    bool high = false;
    size_t k = 0, m = 0;
    std::vector<uint16_t> rows;  // 2 k field elements: M[0][i], then M[1][i]
    // u16 tables on the device: log (GF_ORDER), exp (GF_ORDER), ratio -> i
    // (GF_ORDER, the last entry unused), log M[0][i] (k)
    struct Dev {
        DevBuf tab;
    } dev;
};
template void rs16::detach(rs16_locate_plan*);

// Rows 0 and 1 of M from the engine's own encode of unit vectors, so they are
// exact on every rate path: original i carries the element 1 at element
// position i, i.e. in block i / 32 of a stripe of 64 ceil(k / 32)-byte shards,
// and recovery row j returns M[j][i] there.  Taken in column chunks of at most
// UNIT_BYTES per shard (512 originals each), so the work space stays small: the
// unit array is cleared once, and each chunk sets its ones, encodes, copies
// rows 0 and 1 back and clears its ones again.
static constexpr size_t UNIT_BYTES = 1024;
static int locate_rows(rs16_engine* e, bool high, size_t k, size_t m, std::vector<uint16_t>& rows, rs16_error* err) {
    const size_t per = UNIT_BYTES / 2;
    const size_t Smax = std::min(UNIT_BYTES, 64 * ((k + 31) / 32));
    std::vector<uint8_t> rec(2 * Smax);
    rows.assign(2 * k, 0);
    DevBuf d_unit, d_rec;
    RS16_HIP(d_unit.reserve(k * Smax));
    RS16_HIP(d_rec.reserve(m * Smax));
    hipStream_t s = e->stream;
    if (int rc = e->order(s, err)) return rc;
    // (on the stream the ones are set on: a non-blocking stream does not wait for the null stream)
    RS16_HIP(hipMemsetAsync(d_unit.p, 0, k * Smax, s));
    // (the first chunk is the widest: the engine's scratch grows there or not at all)
    for (size_t i0 = 0; i0 < k; i0 += per) {
        const size_t n = std::min(per, k - i0), S = 64 * ((n + 31) / 32);
        RS16_HIP(launch_locate_unit((uint8_t*)d_unit.p, S, (uint32_t)i0, (uint32_t)n, 1, s));
        if (int rc = encode_stripes(e, high, k, m, S, 1, (const uint8_t*)d_unit.p, 0, (uint8_t*)d_rec.p, 0, s, err))
            return rc;
        RS16_HIP(launch_locate_unit((uint8_t*)d_unit.p, S, (uint32_t)i0, (uint32_t)n, 0, s));
        RS16_HIP(hipMemcpyAsync(rec.data(), d_rec.p, 2 * S, hipMemcpyDeviceToHost, s));
        RS16_HIP(hipStreamSynchronize(s));
        for (size_t j = 0; j < 2; j++)
            for (size_t q = 0; q < n; q++) {
                const size_t at = j * S + 64 * (q / 32) + q % 32;
                rows[j * k + i0 + q] = (uint16_t)(rec[at] | (uint16_t)rec[at + 32] << 8);
            }
    }
    return e->scratch_done(s, err);
}

extern "C" rs16_locate_plan* rs16_locate_plan_new(rs16_engine* eng, int rate, size_t k, size_t m, rs16_error* err) {
    if (!eng) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    bool high;
    if (resolve_rate(rate, k, m, 64, &high, err)) return nullptr;
    // distance 2 detects an error and cannot locate it
    if (m < 2) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    if (eng->activate(err)) return nullptr;
    rs16_locate_plan* p = new (std::nothrow) rs16_locate_plan();
    if (!p) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    p->eng = eng;
    p->high = high, p->k = k, p->m = m;
    eng->locate_plans.push_back(p);
    auto build = [&]() -> int {
        if (int rc = locate_rows(eng, high, k, m, p->rows, err)) return rc;
        const HostTables& t = host_tables();
        std::vector<uint16_t> tab(3 * (size_t)GF_ORDER + k);
        std::copy(t.log.begin(), t.log.end(), tab.begin());
        std::copy(t.exp.begin(), t.exp.end(), tab.begin() + GF_ORDER);
        uint16_t* ratio = tab.data() + 2 * (size_t)GF_ORDER;
        uint16_t* log_m0 = ratio + GF_ORDER;
        std::fill(ratio, ratio + GF_ORDER, (uint16_t)0xFFFF);
        for (size_t i = 0; i < k; i++) {
            const uint16_t a = p->rows[i], b = p->rows[k + i];
            // what the method rests on (MDS: no zero entry, no singular 2 x 2 minor)
            if (a == 0 || b == 0) return set_error(err, RS16_INVALID_ARGUMENT);
            const uint32_t la = t.log[a], lb = t.log[b];
            const uint32_t d = la >= lb ? la - lb : la + GF_MODULUS - lb;
            if (ratio[d] != 0xFFFF) return set_error(err, RS16_INVALID_ARGUMENT);
            ratio[d] = (uint16_t)i;
            log_m0[i] = (uint16_t)la;
        }
        RS16_HIP(p->dev.tab.reserve(tab.size() * 2));
        RS16_HIP(hipMemcpy(p->dev.tab.p, tab.data(), tab.size() * 2, hipMemcpyHostToDevice));
        return RS16_OK;
    };
    if (build()) {
        rs16_locate_plan_free(p);
        return nullptr;
    }
    set_error(err, RS16_OK);
    return p;
}

extern "C" void rs16_locate_plan_free(rs16_locate_plan* p) { free_attached(p, &rs16_engine::locate_plans); }

extern "C" int rs16_locate_plan_rows(rs16_locate_plan* p, uint16_t* out, rs16_error* err) {
    if (!p || !p->eng || !out) return set_error(err, RS16_INVALID_ARGUMENT);
    memcpy(out, p->rows.data(), p->rows.size() * sizeof(uint16_t));
    return set_error(err, RS16_OK);
}

// A work buffer of the locate that must keep its contents between calls: grown
// if needed, *clean reset when that lost them (at once: a later step of the
// call may fail).
static hipError_t keep(DevBuf& b, size_t bytes, bool* clean) {
    if (bytes > b.cap) *clean = false;
    return b.reserve(bytes);
}

// What the heal adds to a locate (nullptr: a locate): the arrays it may write
// are the call's shard arrays, by the mask; the counts are the caller's.
struct Heal {
    int mask;
    uint32_t* counts;
    size_t counts_stride;  // entries
};

// The used range of each stripe's entries of an output array cleared, the bytes
// between the strides left alone.
static hipError_t clear_strided(void* p, size_t stride, size_t used, size_t nstripes, hipStream_t s) {
    if (nstripes == 1 || stride == used) return hipMemsetAsync(p, 0, (nstripes - 1) * stride + used, s);
    return hipMemset2DAsync(p, stride, 0, used, nstripes, s);
}

// All four entry points: nstripes stripes of the plan's geometry, stripe i's
// arrays at + i o_stride / r_stride and its outputs at + i st_stride (bytes) /
// sh_stride (entries) / fx_stride (bytes) (the single calls: one stripe).  The
// engine's buffers hold every stripe's share side by side: both encodes and E at
// their natural strides, nslots copies of the pairs and B candidates per
// stripe, and for the heal B x 64 bytes of fix per stripe and, where the caller
// gave none, status and shard.
static int locate(rs16_locate_plan* p, size_t S, bool batched, size_t nstripes, const void* d_original,
                  size_t o_stride, const void* d_recovery, size_t r_stride, uint8_t* d_status, size_t st_stride,
                  uint32_t* d_shard, size_t sh_stride, void* d_fix, size_t fx_stride, const Heal* heal, void* stream,
                  rs16_error* err) {
    if (!p || !p->eng) return set_error(err, RS16_INVALID_ARGUMENT);
    const size_t k = p->k, m = p->m;
    const bool high = p->high;
    if (int rc = rs16_validate(high ? RS16_RATE_HIGH : RS16_RATE_LOW, k, m, S, err)) return rc;
    if (!batched) o_stride = k * S, r_stride = m * S;  // (one stripe: the kernels still ask for whole strides)
    if (!d_original || !d_recovery || !shard_aligned(d_original) || !shard_aligned(d_recovery) ||
        (!heal && (!d_status || !d_shard)))
        return set_error(err, RS16_INVALID_ARGUMENT);
    if (heal && (heal->mask == 0 || (heal->mask & ~(RS16_HEAL_ORIGINAL | RS16_HEAL_RECOVERY)) || !heal->counts))
        return set_error(err, RS16_INVALID_ARGUMENT);
    const size_t B = S / 64;
    if (batched && (!batch_layout_ok(k, m, S, nstripes, o_stride, r_stride) || (d_status && st_stride < B) ||
                    (d_shard && sh_stride < B) || (d_fix && fx_stride < 64 * B) ||
                    (heal && heal->counts_stride < 4) || nstripes > 65535))
        return set_error(err, RS16_INVALID_ARGUMENT);
    if (nstripes == 0) return set_error(err, RS16_OK);
    rs16_engine* e = p->eng;
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    RS16_HIP(e->ws_rep.reserve(nstripes * m * S));
    RS16_HIP(e->ws_loc_rep.reserve(nstripes * m * S));
    // per stripe B candidates and, for a heal without the caller's, B shard entries and B status bytes
    RS16_HIP(e->ws_loc_cand.reserve(nstripes * B * (heal ? 9 : 4)));
    if (heal) RS16_HIP(e->ws_loc_fix.reserve(nstripes * B * 64));
    RS16_HIP(keep(e->ws_loc_e, nstripes * k * S, &e->loc_clean));
    // copies of the scan's pairs, which its row walkers spread over: shards up
    // to 64 KiB have few lanes per row and many walkers per column
    const uint32_t nslots = S <= 65536 ? LOCATE_MAX_SLOTS : 1;
    RS16_HIP(keep(e->ws_loc_acc, nstripes * nslots * (S / 2) * 8, &e->loc_clean));
    // Both are zero as a whole between calls, so a call may lay its stripes
    // over them as it likes: one stripe after a batch, a batch after one stripe.
    if (!e->loc_clean) {
        RS16_HIP(hipMemsetAsync(e->ws_loc_e.p, 0, e->ws_loc_e.cap, s));
        RS16_HIP(hipMemsetAsync(e->ws_loc_acc.p, 0, e->ws_loc_acc.cap, s));
    }
    e->loc_clean = false;  // until the confirm kernel, which puts the last of it back, is enqueued
    const uint16_t* tab = (const uint16_t*)p->dev.tab.p;
    LocateArgs a{};
    a.enc = (const uint8_t*)e->ws_rep.p, a.bs_enc = m * S;
    a.rec = (const uint8_t*)d_recovery, a.bs_rec = r_stride;
    a.enc2 = (const uint8_t*)e->ws_loc_rep.p, a.bs_enc2 = m * S;
    a.E = (uint8_t*)e->ws_loc_e.p, a.bs_E = k * S;
    a.acc = (unsigned long long*)e->ws_loc_acc.p, a.bs_acc = nslots * (S / 2);
    a.nslots = nslots;
    a.cand = (uint32_t*)e->ws_loc_cand.p, a.bs_cand = B;
    a.log = tab, a.exp = tab + GF_ORDER, a.ratio = tab + 2 * (size_t)GF_ORDER, a.log_m0 = tab + 3 * (size_t)GF_ORDER;
    a.status = d_status, a.bs_status = st_stride;
    a.shard = d_shard, a.bs_shard = sh_stride;
    a.fix = (uint8_t*)d_fix, a.bs_fix = fx_stride;
    if (heal) {
        if (!d_shard) a.shard = a.cand + nstripes * B, a.bs_shard = B;
        if (!d_status) a.status = (uint8_t*)(a.cand + 2 * nstripes * B), a.bs_status = B;
        a.fix = (uint8_t*)e->ws_loc_fix.p, a.bs_fix = 64 * B;
        a.orig_w = heal->mask & RS16_HEAL_ORIGINAL ? (uint8_t*)d_original : nullptr, a.bs_orig = o_stride;
        a.rec_w = heal->mask & RS16_HEAL_RECOVERY ? (uint8_t*)d_recovery : nullptr;
        a.counts = heal->counts, a.bs_counts = heal->counts_stride;
    }
    a.S = S, a.k = (uint32_t)k, a.m = (uint32_t)m, a.blocks = (uint32_t)B, a.nstripes = (uint32_t)nstripes;
    // the syndromes' first half, then what they say ...
    if (int rc = encode_stripes(e, high, k, m, S, nstripes, (const uint8_t*)d_original, o_stride,
                                (uint8_t*)e->ws_rep.p, a.bs_enc, s, err))
        return rc;
    if (int rc = e->profiled(PROF_LOCATE_SCAN, s, err, [&](uint64_t*) { return launch_locate_scan(a, s); })) return rc;
    if (int rc = e->profiled(PROF_LOCATE_DECIDE, s, err, [&](uint64_t*) { return launch_locate_decide(a, s); }))
        return rc;
    // ... and the check of every ORIGINAL candidate against all m rows.  Always
    // run: whether any block names an original is known on the device only.
    if (int rc = encode_stripes(e, high, k, m, S, nstripes, a.E, a.bs_E, (uint8_t*)e->ws_loc_rep.p, a.bs_enc2, s, err))
        return rc;
    if (int rc = e->profiled(PROF_LOCATE_CONFIRM, s, err, [&](uint64_t*) { return launch_locate_confirm(a, s); }))
        return rc;
    e->loc_clean = true;
    if (heal) {
        // after both encodes and every read of the stored shards: the fix goes in place
        RS16_HIP(clear_strided(heal->counts, 4 * heal->counts_stride, 16, nstripes, s));
        if (int rc = e->profiled(PROF_LOCATE_APPLY, s, err, [&](uint64_t*) { return launch_locate_apply(a, s); }))
            return rc;
    }
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_locate_device(rs16_locate_plan* p, size_t S, const void* d_original, const void* d_recovery,
                                  uint8_t* d_block_status, uint32_t* d_block_shard, void* d_block_fix, void* stream,
                                  rs16_error* err) {
    return locate(p, S, false, 1, d_original, 0, d_recovery, 0, d_block_status, S / 64, d_block_shard, S / 64,
                  d_block_fix, S, nullptr, stream, err);
}

extern "C" int rs16_locate_device_batch(rs16_locate_plan* p, size_t S, size_t nstripes, const void* d_original,
                                        size_t original_stride, const void* d_recovery, size_t recovery_stride,
                                        uint8_t* d_block_status, size_t status_stride, uint32_t* d_block_shard,
                                        size_t shard_stride, void* d_block_fix, size_t fix_stride, void* stream,
                                        rs16_error* err) {
    return locate(p, S, true, nstripes, d_original, original_stride, d_recovery, recovery_stride, d_block_status,
                  status_stride, d_block_shard, shard_stride, d_block_fix, fix_stride, nullptr, stream, err);
}

extern "C" int rs16_heal_device(rs16_locate_plan* p, size_t S, void* d_original, void* d_recovery, int heal_mask,
                                uint8_t* d_block_status, uint32_t* d_block_shard, uint32_t* d_counts, void* stream,
                                rs16_error* err) {
    const Heal heal{heal_mask, d_counts, 4};
    return locate(p, S, false, 1, d_original, 0, d_recovery, 0, d_block_status, S / 64, d_block_shard, S / 64, nullptr,
                  0, &heal, stream, err);
}

extern "C" int rs16_heal_device_batch(rs16_locate_plan* p, size_t S, size_t nstripes, void* d_original,
                                      size_t original_stride, void* d_recovery, size_t recovery_stride, int heal_mask,
                                      uint8_t* d_block_status, size_t status_stride, uint32_t* d_block_shard,
                                      size_t shard_stride, uint32_t* d_counts, size_t counts_stride, void* stream,
                                      rs16_error* err) {
    const Heal heal{heal_mask, d_counts, counts_stride};
    return locate(p, S, true, nstripes, d_original, original_stride, d_recovery, recovery_stride, d_block_status,
                  status_stride, d_block_shard, shard_stride, nullptr, 0, &heal, stream, err);
}

// The scan launch's shape {cw, rsub, gx, gy, rows_per_wg} for nstripes stripes
// of recovery_count rows of shard_bytes (include/rs16.h); 0, or -1 for sizes no
// locate takes.  Host arithmetic only.
extern "C" int rs16_host_locate_scan_shape(size_t S, size_t m, size_t nstripes, uint32_t out[5]) {
    if (!out || S == 0 || S % 64 || S >= ((size_t)1 << 32) || m == 0 || m >= GF_ORDER || nstripes == 0 ||
        nstripes > 65535)
        return -1;
    const LocateScanShape sh = locate_scan_shape(S, (uint32_t)m, (uint32_t)nstripes);
    out[0] = sh.cw, out[1] = sh.rsub, out[2] = sh.gx, out[3] = sh.gy, out[4] = sh.rows_per_wg;
    return 0;
}
