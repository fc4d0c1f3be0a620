// TEST INFRASTRUCTURE: the launcher of ONE generated quotient kernel (zk_expr_specialised_source) under the emulator.
// The including translation unit is  #include "emu_hip.h", the generated source with its kernel renamed
// (#define zk_expr_jit <ZK_EXPR_JIT_KERNEL>), then this header with ZK_EXPR_JIT_KERNEL and ZK_EXPR_JIT_ENTRY defined
// (tests/test_expr_corpus.py writes it).  The grid is the caller's: 64 lanes per block, as the library launches it.
#pragma once

extern "C" __attribute__((visibility("default"))) void ZK_EXPR_JIT_ENTRY(const void* const* cols, const void* consts, unsigned log_n,
                                                                         unsigned rot_scale, void* out, unsigned grid) {
    emu::launch(grid, 64, 0, [&]() {
        ZK_EXPR_JIT_KERNEL((const zk::Fe<F>* const*)cols, (const zk::Fe<F>*)consts, log_n, rot_scale, (zk::Fe<F>*)out);
    });
}
