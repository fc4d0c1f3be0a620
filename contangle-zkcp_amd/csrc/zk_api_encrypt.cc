// C ABI, EncryptCircuit: the per-element section of the assignment and the plaintext of a byte string.
#include "zk_api_common.h"
#include "zk_ntt_decl.h"

using namespace zk;

namespace {
constexpr uint64_t ENCRYPT_MAX_N = 1ull << 40;
}  // namespace

extern "C" {

API int zk_encrypt_witness_device(zk_field_t f, const void* msg_dev, uint64_t msg_len, uint64_t n, const void* dh_mont_host, void* c2_dev, void* m_dev,
                                  void* b_dev, void* k_dev, void* stream) {
    if (!dh_mont_host || msg_len > n || n > ENCRYPT_MAX_N || (msg_len && (!msg_dev || !aligned16(msg_dev)))) return ZK_ERR_INVALID_ARG;
    void* outs[4] = {c2_dev, m_dev, b_dev, k_dev};
    if (n) {
        for (int i = 0; i < 4; i++) {
            if (!outs[i] || !aligned16(outs[i])) return ZK_ERR_INVALID_ARG;
            for (int j = 0; j < i; j++)
                if (spans_overlap(outs[i], n * 32, outs[j], n * 32)) return ZK_ERR_INVALID_ARG;
            if (msg_len && spans_overlap(outs[i], n * 32, msg_dev, msg_len * 32)) return ZK_ERR_INVALID_ARG;
        }
    }
    FIELD_SWITCH(f, {
        if (!canonical_elems<F>(dh_mont_host, 1)) return ZK_ERR_INVALID_ARG;
    });
    DEVICE_ENTRY(c2_dev);
    FIELD_SWITCH(f, {
        Fe<F> dh;
        host_load(dh, dh_mont_host);
        return FieldLaunch<F>::encrypt_witness_run((const Fe<F>*)msg_dev, msg_len, n, dh, (Fe<F>*)c2_dev, (Fe<F>*)m_dev, (Fe<F>*)b_dev, (Fe<F>*)k_dev,
                                                   (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}

API int zk_plaintext_from_bytes_device(zk_field_t f, const uint8_t* bytes_dev, uint64_t len, void* out_dev, uint64_t n, void* stream) {
    if ((int)f < 0 || (int)f > (int)ZK_FR_BLS12_381 || n > ENCRYPT_MAX_N || len > ENCRYPT_MAX_N || (n && (!out_dev || !aligned16(out_dev))) ||
        (n && len && !bytes_dev))
        return ZK_ERR_INVALID_ARG;
    const uint64_t read = len < n ? len : n;          // bytes past n are never read (upstream drops them)
    if (n && read && spans_overlap(out_dev, n * 32, bytes_dev, read)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out_dev);
    FIELD_SWITCH(f, return FieldLaunch<F>::plaintext_from_bytes_run(bytes_dev, read, (Fe<F>*)out_dev, n, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

}  // extern "C"
