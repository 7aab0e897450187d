// rs16_api_update.cpp -- C ABI (include/rs16.h): the delta update of recovery
// shards (rs16_update_plan).
#include "rs16_api.hpp"

using namespace rs16;

// ---------------------------------------------------------------------------
// Delta update of recovery shards (include/rs16.h "Partial-stripe writes").
// The encode is GF(2^16)-linear per element position: recovery_j = sum_i
// M[j][i] original_i.  A plan holds the columns of M of its n originals.  The
// 32 elements of a 64-byte block are independent codewords, so ONE encode of a
// k x 64 B stripe yields them: element e of the block is the field element 1
// in shard indices[e] and 0 everywhere else, and element e of recovery row j
// comes out as M[j][indices[e]] -- by the engine's own encode of that rate,
// whatever path it takes.
// ---------------------------------------------------------------------------
struct rs16_update_plan {
    rs16_engine* eng;  // nullptr once the engine was freed (detached)
    size_t k = 0, m = 0, n = 0;
    std::vector<uint16_t> coef;  // m x n field elements, coef[j n + e] = M[j][indices[e]]
    struct Dev {
        DevBuf idx;  // m x n d_mul_tab entries of them (ZERO_ENTRY for 0)
    } dev;
};
template void rs16::detach(rs16_update_plan*);

// The unit-vector encode: coef[j n + e] = M[j][indices[e]].
static int update_coefficients(rs16_engine* e, bool high, size_t k, size_t m, const size_t* indices, size_t n,
                               std::vector<uint16_t>& coef, rs16_error* err) {
    const size_t S = 64;
    std::vector<uint8_t> unit(k * S, 0), rec(m * S);
    for (size_t el = 0; el < n; el++) unit[indices[el] * S + el] = 1;  // low byte 1, high byte 0
    DevBuf d_unit, d_rec;
    RS16_HIP(d_unit.reserve(k * S));
    RS16_HIP(d_rec.reserve(m * S));
    RS16_HIP(hipMemcpy(d_unit.p, unit.data(), k * S, hipMemcpyHostToDevice));
    hipStream_t s = e->stream;
    if (int rc = e->order(s, err)) return rc;
    if (int rc = encode_stripes(e, high, k, m, S, 1, (const uint8_t*)d_unit.p, 0, (uint8_t*)d_rec.p, 0, s, err))
        return rc;
    if (int rc = e->scratch_done(s, err)) return rc;
    RS16_HIP(hipStreamSynchronize(s));
    RS16_HIP(hipMemcpy(rec.data(), d_rec.p, m * S, hipMemcpyDeviceToHost));
    coef.resize(m * n);
    for (size_t j = 0; j < m; j++)
        for (size_t el = 0; el < n; el++)
            coef[j * n + el] = (uint16_t)(rec[j * S + el] | (uint16_t)rec[j * S + 32 + el] << 8);
    return RS16_OK;
}

extern "C" rs16_update_plan* rs16_update_plan_new(rs16_engine* eng, int rate, size_t k, size_t m,
                                                  const size_t* indices, size_t n, rs16_error* err) {
    if (!eng) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    bool high;
    if (resolve_rate(rate, k, m, 64, &high, err)) return nullptr;
    if (n == 0 || n > RS16_UPDATE_MAX_SHARDS || !indices) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    for (size_t a = 0; a < n; a++)
        if (indices[a] >= k) return set_error(err, RS16_INVALID_ORIGINAL_SHARD_INDEX, k, indices[a]), nullptr;
    for (size_t a = 0; a < n; a++)
        for (size_t b = 0; b < a; b++)
            if (indices[a] == indices[b])
                return set_error(err, RS16_DUPLICATE_ORIGINAL_SHARD_INDEX, indices[a]), nullptr;
    if (eng->activate(err)) return nullptr;
    rs16_update_plan* p = new (std::nothrow) rs16_update_plan();
    if (!p) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    p->eng = eng;
    p->k = k, p->m = m, p->n = n;
    eng->update_plans.push_back(p);
    auto build = [&]() -> int {
        if (int rc = update_coefficients(eng, high, k, m, indices, n, p->coef, err)) return rc;
        const HostTables& t = host_tables();
        std::vector<uint32_t> entry(m * n);
        for (size_t i = 0; i < m * n; i++) entry[i] = p->coef[i] ? (uint32_t)t.log[p->coef[i]] : ZERO_ENTRY;
        RS16_HIP(p->dev.idx.reserve(m * n * 4));
        // a host copy, complete before any launch reads the array on the scalar path
        RS16_HIP(hipMemcpy(p->dev.idx.p, entry.data(), m * n * 4, hipMemcpyHostToDevice));
        return RS16_OK;
    };
    if (build()) {
        rs16_update_plan_free(p);
        return nullptr;
    }
    set_error(err, RS16_OK);
    return p;
}

extern "C" void rs16_update_plan_free(rs16_update_plan* p) { free_attached(p, &rs16_engine::update_plans); }

extern "C" size_t rs16_update_plan_count(const rs16_update_plan* p) { return p ? p->n : 0; }

extern "C" int rs16_update_plan_coefficients(rs16_update_plan* p, uint16_t* out, rs16_error* err) {
    if (!p || !p->eng || !out) return set_error(err, RS16_INVALID_ARGUMENT);
    memcpy(out, p->coef.data(), p->coef.size() * sizeof(uint16_t));
    return set_error(err, RS16_OK);
}

extern "C" int rs16_update_device(rs16_update_plan* p, size_t S, const void* d_delta, void* d_recovery,
                                  size_t recovery_pos, size_t recovery_n, void* stream, rs16_error* err) {
    if (!p || !p->eng) return set_error(err, RS16_INVALID_ARGUMENT);
    if (S == 0 || (S & 63) != 0) return set_error(err, RS16_INVALID_SHARD_SIZE, S);
    if (recovery_pos > p->m || recovery_n > p->m - recovery_pos) return set_error(err, RS16_INVALID_ARGUMENT);
    if (recovery_n == 0) return set_error(err, RS16_OK);
    // (quads per row as a 32-bit count)
    if (!d_delta || !d_recovery || S / 8 > 0xFFFFFFFFu || !shard_aligned(d_delta) || !shard_aligned(d_recovery))
        return set_error(err, RS16_INVALID_ARGUMENT);
    rs16_engine* e = p->eng;
    if (int rc = e->activate(err)) return rc;
    UpdateArgs a{};
    a.rec = (uint8_t*)d_recovery;
    a.delta = (const uint8_t*)d_delta;
    a.idx = (const uint32_t*)p->dev.idx.p;
    a.mul_tab = e->d_mul_tab.as<uint32_t>();
    a.S = S;
    a.qrow = (uint32_t)(S / 8);
    a.row0 = (uint32_t)recovery_pos;
    a.rows = (uint32_t)recovery_n;
    RS16_HIP(launch_update(a, (uint32_t)p->n, e->pick(stream)));
    return set_error(err, RS16_OK);
}

// (rows - 1) pitch + width <= stride, without overflow (rows >= 1, pitch >= width)
static bool rows_fit(size_t rows, size_t pitch, size_t width, size_t stride) {
    return stride >= width && (stride - width) / pitch >= rows - 1;
}

extern "C" int rs16_update_device_batch(rs16_update_plan* p, size_t width, size_t nstripes, const void* d_delta,
                                        size_t delta_pitch, size_t delta_stride, void* d_recovery,
                                        size_t recovery_pitch, size_t recovery_stride, size_t recovery_pos,
                                        size_t recovery_n, void* stream, rs16_error* err) {
    if (!p || !p->eng) return set_error(err, RS16_INVALID_ARGUMENT);
    if (width == 0 || (width & 63) != 0) return set_error(err, RS16_INVALID_SHARD_SIZE, width);
    if (recovery_pos > p->m || recovery_n > p->m - recovery_pos) return set_error(err, RS16_INVALID_ARGUMENT);
    if (recovery_n == 0 || nstripes == 0) return set_error(err, RS16_OK);
    if (!d_delta || !d_recovery || !shard_aligned(d_delta) || !shard_aligned(d_recovery))
        return set_error(err, RS16_INVALID_ARGUMENT);
    if ((delta_pitch & 63) != 0 || (recovery_pitch & 63) != 0 || delta_pitch < width || recovery_pitch < width)
        return set_error(err, RS16_INVALID_ARGUMENT);
    // (stripes that overlap would race: each is read and written by waves of its own)
    if (nstripes > 1 && ((delta_stride & 63) != 0 || (recovery_stride & 63) != 0 ||
                         !rows_fit(recovery_n, recovery_pitch, width, recovery_stride) ||
                         !rows_fit(p->n, delta_pitch, width, delta_stride)))
        return set_error(err, RS16_INVALID_ARGUMENT);
    // (the heal's cap; a lane's offset inside a row is a 32-bit count)
    if (nstripes > 65535 || width > 0xFFFFFFFFu || delta_pitch > 0xFFFFFFFFu || recovery_pitch > 0xFFFFFFFFu)
        return set_error(err, RS16_INVALID_ARGUMENT);
    rs16_engine* e = p->eng;
    if (int rc = e->activate(err)) return rc;
    UpdateBatchArgs a{};
    a.rec = (uint8_t*)d_recovery;
    a.delta = (const uint8_t*)d_delta;
    a.idx = (const uint32_t*)p->dev.idx.p;
    a.mul_tab = e->d_mul_tab.as<uint32_t>();
    a.delta_pitch = delta_pitch, a.rec_pitch = recovery_pitch;
    // (one stripe has no stride: whatever the caller passed is not used)
    a.delta_stride = nstripes > 1 ? delta_stride : 0, a.rec_stride = nstripes > 1 ? recovery_stride : 0;
    a.qrow = (uint32_t)(width / 8);
    a.row0 = (uint32_t)recovery_pos;
    a.rows = (uint32_t)recovery_n;
    a.nstripes = (uint32_t)nstripes;
    RS16_HIP(launch_update_batch(a, (uint32_t)p->n, e->pick(stream)));
    return set_error(err, RS16_OK);
}
