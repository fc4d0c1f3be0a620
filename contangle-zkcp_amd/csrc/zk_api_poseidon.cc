// C ABI, Poseidon: the registry of parameter sets with their per-device tables, sponge hashing, the Merkle tree over it and the
// ElGamal stream's vector addition.
#include "zk_api_common.h"
#include "zk_ntt_decl.h"
#include "zk_poseidon_kernels.h"

using namespace zk;

namespace {
// Poseidon parameter sets (zk_poseidon_create): the table [ark | mds | init] on the host, for the host twin and as the source of the
// one copy per device that the first *_device call there uploads.  Handles need no device and outlive zk_shutdown (their device
// copies do not).
struct PoseidonEntry {
    int field = 0;
    PoseidonShape shape;
    std::vector<uint64_t> tbl;            // 4 words per element
    std::map<int, void*> dev;             // device index -> table
};
std::mutex g_pos_mu;
std::map<uint64_t, std::shared_ptr<PoseidonEntry>> g_poseidon;
uint64_t g_next_poseidon = 1;
void free_poseidon_tables(PoseidonEntry& e) {   // (g.mu and g_pos_mu held)
    for (auto& kv : e.dev)
        if (kv.first < (int)g.devs.size()) {
            hipSetDevice(g.devs[kv.first]->device);
            hipDeviceSynchronize();
            hipFree(kv.second);
        }
    e.dev.clear();
}

int find_poseidon(uint64_t handle, std::shared_ptr<PoseidonEntry>* out) {
    std::lock_guard<std::mutex> lk(g_pos_mu);
    auto it = g_poseidon.find(handle);
    if (it == g_poseidon.end()) return ZK_ERR_BAD_HANDLE;
    *out = it->second;
    return ZK_OK;
}
// the handle's table on the calling device, uploaded at the first use there (dc.mu held)
int poseidon_table(PoseidonEntry& e, DeviceCtx& dc, const void** out) {
    std::lock_guard<std::mutex> lk(g_pos_mu);
    auto it = e.dev.find(dc.index);
    if (it == e.dev.end()) {
        void* p = nullptr;
        const size_t bytes = e.tbl.size() * sizeof(uint64_t);
        HIP_TRY(hipMalloc(&p, bytes));
        if (hipMemcpy(p, e.tbl.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(p);
            return ZK_ERR_HIP;
        }
        it = e.dev.emplace(dc.index, p).first;
    }
    *out = it->second;
    return ZK_OK;
}
}  // namespace

namespace zk {
void poseidon_release_tables() {   // zk_shutdown, g.mu held: the handles stay, their device copies go
    std::lock_guard<std::mutex> lkp(g_pos_mu);
    for (auto& kv : g_poseidon) free_poseidon_tables(*kv.second);
}
}  // namespace zk

extern "C" {

// ---- Poseidon, the Merkle tree over it, the ElGamal stream (zk_poseidon.inl) ----
API int zk_poseidon_create(zk_field_t f, uint32_t width, uint32_t rate, uint32_t rate_offset, uint32_t full_rounds, uint32_t partial_rounds,
                           uint64_t alpha, const void* ark_mont_host, const void* mds_mont_host, const void* init_mont_host, uint64_t* handle_out) {
    if (!ark_mont_host || !mds_mont_host || !handle_out || width < POSEIDON_MIN_WIDTH || width > POSEIDON_MAX_WIDTH || rate == 0 || rate > width ||
        rate_offset > width - rate || (full_rounds & 1) || full_rounds > POSEIDON_MAX_ROUNDS || partial_rounds > POSEIDON_MAX_ROUNDS ||
        full_rounds + partial_rounds == 0 || full_rounds + partial_rounds > POSEIDON_MAX_ROUNDS || alpha == 0)
        return ZK_ERR_INVALID_ARG;
    const size_t n_ark = (size_t)(full_rounds + partial_rounds) * width, n_mds = (size_t)width * width;
    FIELD_SWITCH(f, {
        if (!canonical_elems<F>(ark_mont_host, n_ark) || !canonical_elems<F>(mds_mont_host, n_mds) ||
            (init_mont_host && !canonical_elems<F>(init_mont_host, width)))
            return ZK_ERR_INVALID_ARG;
    });
    auto e = std::make_shared<PoseidonEntry>();
    e->field = (int)f;
    e->shape = PoseidonShape{width, rate, rate_offset, full_rounds, partial_rounds, (uint32_t)(63 - __builtin_clzll(alpha)), alpha};
    e->tbl.assign((n_ark + n_mds + width) * 4, 0);
    memcpy(e->tbl.data(), ark_mont_host, n_ark * 32);
    memcpy(e->tbl.data() + n_ark * 4, mds_mont_host, n_mds * 32);
    if (init_mont_host) memcpy(e->tbl.data() + (n_ark + n_mds) * 4, init_mont_host, (size_t)width * 32);
    std::lock_guard<std::mutex> lk(g_pos_mu);
    *handle_out = g_next_poseidon;
    g_poseidon[g_next_poseidon++] = e;
    return ZK_OK;
}
API int zk_poseidon_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk0(g.mu);
    std::lock_guard<std::mutex> lk(g_pos_mu);
    auto it = g_poseidon.find(handle);
    if (it == g_poseidon.end()) return ZK_ERR_BAD_HANDLE;
    free_poseidon_tables(*it->second);
    g_poseidon.erase(it);
    return ZK_OK;
}
API int zk_poseidon_permute_host(uint64_t handle, void* states_mont_host, uint64_t count) {
    if (!states_mont_host) return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    FIELD_SWITCH((zk_field_t)e->field, return FieldLaunch<F>::poseidon_permute_host_run(e->shape, (const Fe<F>*)e->tbl.data(), (Fe<F>*)states_mont_host, count));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_hash_host(uint64_t handle, const void* in_mont_host, uint32_t arity, uint64_t count, void* out_mont_host) {
    if (!in_mont_host || !out_mont_host || arity == 0 || arity > POSEIDON_MAX_ARITY || count > (1ull << 48) ||
        spans_overlap(in_mont_host, count * arity * 32, out_mont_host, count * 32))
        return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    FIELD_SWITCH((zk_field_t)e->field, return FieldLaunch<F>::poseidon_hash_host_run(e->shape, (const Fe<F>*)e->tbl.data(), (const Fe<F>*)in_mont_host, arity, count,
                                                                        (Fe<F>*)out_mont_host));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_permute_device(uint64_t handle, void* states_dev, uint64_t count, void* stream) {
    if (!states_dev || !aligned16(states_dev) || count > (1ull << 48)) return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    DEVICE_ENTRY(states_dev);
    const void* tbl = nullptr;
    ZK_TRY(poseidon_table(*e, dc, &tbl));
    FIELD_SWITCH((zk_field_t)e->field, return FieldLaunch<F>::poseidon_permute_run(e->shape, (const Fe<F>*)tbl, (Fe<F>*)states_dev, count, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_hash_device(uint64_t handle, const void* in_dev, uint32_t arity, uint64_t count, void* out_dev, void* stream) {
    if (!in_dev || !out_dev || !aligned16(in_dev) || !aligned16(out_dev) || arity == 0 || arity > POSEIDON_MAX_ARITY || count > (1ull << 48) ||
        spans_overlap(in_dev, count * arity * 32, out_dev, count * 32))
        return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    DEVICE_ENTRY(out_dev);
    const void* tbl = nullptr;
    ZK_TRY(poseidon_table(*e, dc, &tbl));
    FIELD_SWITCH((zk_field_t)e->field,
                 return FieldLaunch<F>::poseidon_hash_run(e->shape, (const Fe<F>*)tbl, (const Fe<F>*)in_dev, arity, count, (Fe<F>*)out_dev, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_merkle_tree_device(uint64_t handle, const void* leaves_dev, uint32_t leaf_arity, uint32_t log_n, void* nodes_dev, void* stream) {
    if (!leaves_dev || !nodes_dev || !aligned16(leaves_dev) || !aligned16(nodes_dev) || leaf_arity == 0 || leaf_arity > POSEIDON_MAX_ARITY || log_n == 0 ||
        log_n > MERKLE_MAX_LOG_N || spans_overlap(leaves_dev, ((uint64_t)leaf_arity << log_n) * 32, nodes_dev, ((2ull << log_n) - 1) * 32))
        return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    DEVICE_ENTRY(nodes_dev);
    const void* tbl = nullptr;
    ZK_TRY(poseidon_table(*e, dc, &tbl));
    FIELD_SWITCH((zk_field_t)e->field,
                 return FieldLaunch<F>::poseidon_tree_run(e->shape, (const Fe<F>*)tbl, (const Fe<F>*)leaves_dev, leaf_arity, log_n, (Fe<F>*)nodes_dev, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_merkle_paths_device(zk_field_t f, const void* nodes_dev, uint32_t log_n, const uint64_t* indices_host, uint64_t count, void* out_dev,
                               void* stream) {
    if (!nodes_dev || !indices_host || !out_dev || !aligned16(nodes_dev) || !aligned16(out_dev) || log_n == 0 || log_n > MERKLE_MAX_LOG_N ||
        count > (1ull << 32) || spans_overlap(nodes_dev, ((2ull << log_n) - 1) * 32, out_dev, count * log_n * 32) || (int)f < 0 ||
        (int)f > (int)ZK_FR_BLS12_381)
        return ZK_ERR_INVALID_ARG;
    for (uint64_t c = 0; c < count; c++)
        if (indices_host[c] >> log_n) return ZK_ERR_INVALID_ARG;       // a lane must never read past the tree
    DEVICE_ENTRY(nodes_dev);
    FIELD_SWITCH(f, return FieldLaunch<F>::merkle_paths_run((const Fe<F>*)nodes_dev, log_n, indices_host, count, (Fe<F>*)out_dev, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_add_scalar_device(zk_field_t f, void* out_dev, const void* a_dev, uint64_t n, const void* scalar_mont_host, void* stream) {
    if (!out_dev || !a_dev || !scalar_mont_host || !aligned16(out_dev) || !aligned16(a_dev) || n > (1ull << 48) ||
        (out_dev != a_dev && spans_overlap(out_dev, n * 32, a_dev, n * 32)))
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (!canonical_elems<F>(scalar_mont_host, 1)) return ZK_ERR_INVALID_ARG;
    });
    DEVICE_ENTRY(out_dev);
    FIELD_SWITCH(f, {
        Fe<F> s;
        host_load(s, scalar_mont_host);
        return FieldLaunch<F>::vec_add_scalar_run((Fe<F>*)out_dev, (const Fe<F>*)a_dev, n, s, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}

}  // extern "C"
