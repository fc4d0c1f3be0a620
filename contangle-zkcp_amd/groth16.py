"""Mirror of ark-groth16 0.3 `create_proof` around the device path (call sites
lib/src/zk/encryption.rs:76, verifiable_encryption.rs:92, sample_entries.rs:86, property.rs:133):

  R1csMatrix                 ark-relations 0.3 ConstraintMatrices rows, resident in CSR form (fixed per circuit)
  witness_map                r1cs_to_qap.rs R1CStoQAP::witness_map from the full assignment: 3 sparse mat-vecs + 7 NTTs + glue
  Prover.prove(z, r, s)      prover.rs create_proof_with_reduction_and_matrices: witness map -> h ; the five MSMs
                             (submitted back to back, collected afterwards) ; assembly of A, B, C ; ark_to_bytes(proof)
  generate_parameters        generator.rs generate_parameters (what the reference's `compile` runs through Groth16::setup,
                             lib/src/zk/encryption.rs:169): Lagrange coefficients at tau, the QAP at tau from the resident
                             matrices (three TRANSPOSED sparse mat-vecs), the key scalars, the fixed-base multiplications;
                             -> Parameters: point vectors on the device, serialize_unchecked() = the key file `compile` writes
  generate_random_parameters the same with the five trapdoor scalars drawn from `secrets`
  VerifyingKey / verify      verifier.rs (the buyer's side: lib/src/zk/encryption.rs:152, sample_entries.rs:126, property.rs:177 after
                             read_verifying_key): VerifyingKey.deserialize = the CHECKED decode of the key file, gamma_abc_g1 on the
                             device (one lane per point: square root, subgroup test) and resident from then on; prepare_inputs = one
                             MSM over it; prepare_verifying_key / verify_proof_with_prepared_inputs = the pairing check on the host

The blinding scalars r, s are arguments: upstream draws them from the caller's RNG, so a proof is reproducible bit for
bit only when the unmodified Rust prover drives the FFI (SURVEY 7 "hard parts"); everything before them is deterministic.
"""
import ctypes
import secrets

import numpy as np

from . import (Bases, _call, _np64, _ptr, ark_serialize, backend_info, base_limbs, curve_id, field_id, field_modulus, fixed_base_msm_device, i32,
               load, msm_submit, ptr, u32, u64, vec_op, vp)

class Assembly(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query0", "b_g1_query0",
                                                "b_g2_query0", "a_acc", "b_g1_acc", "l_acc", "h_acc", "b_g2_acc", "r", "s")]


class VkPoints(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2")]


SIGNATURES = {
    "zk_r1cs_matrix_upload": [i32, vp, vp, vp, u64, u64, ptr(u64)],
    "zk_r1cs_matrix_free": [u64],
    "zk_r1cs_matvec_device": [u64, vp, vp, u64, vp],
    "zk_groth16_witness_map_r1cs_device": [i32, u64, u64, u64, vp, u64, u32, vp, vp, vp, vp],
    "zk_groth16_assemble_proof": [i32, ptr(Assembly), vp, vp, vp],
    "zk_r1cs_matvec_transposed_device": [u64, vp, u64, vp, u64, vp],
    "zk_lagrange_coefficients_device": [i32, u32, vp, vp, vp, vp],
    "zk_groth16_qap_at_device": [i32, u64, u64, u64, u64, u32, vp, vp, vp, vp, u64, vp, vp],
    "zk_groth16_key_scalars_device": [i32, vp, vp, vp, u64, u64, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "zk_pairing_product": [i32, vp, vp, u64, vp],
    "zk_groth16_verify": [i32, ptr(VkPoints), vp, vp, vp, vp, vp, ptr(u64)],
    "zk_groth16_prepare_inputs": [i32, u64, vp, u64, vp, u64, vp, vp],
    "zk_r1cs_first_unsatisfied_device": [i32, u64, u64, u64, vp, u64, vp, u64, ptr(u64), vp],
}
PROVER_EXPORTS = list(SIGNATURES)
_lib = load         # the bound handle (tests and tools take it for raw calls)


class R1csMatrix:
    """rows: list of rows, a row = list of (coefficient as Montgomery u64[4], variable index)  -- or CSR arrays directly"""

    def __init__(self, field, rows=None, n_cols=None, csr=None):
        self.field = field_id(field)
        if csr is None:
            row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
            for i, row in enumerate(rows):
                row_ptr[i + 1] = row_ptr[i] + len(row)
            nnz = int(row_ptr[-1])
            col = np.zeros(max(nnz, 1), dtype=np.uint32)
            val = np.zeros((max(nnz, 1), 4), dtype=np.uint64)
            k = 0
            for row in rows:
                for c, j in row:
                    val[k] = c
                    col[k] = j
                    k += 1
        else:
            row_ptr, col, val = (np.ascontiguousarray(csr[0], dtype=np.uint64), np.ascontiguousarray(csr[1], dtype=np.uint32),
                                 _np64(csr[2]))
        self.n_rows, self.n_cols = int(row_ptr.shape[0]) - 1, int(n_cols)
        h = ctypes.c_uint64(0)
        _call("zk_r1cs_matrix_upload", self.field, _ptr(row_ptr), _ptr(col), _ptr(val), self.n_rows, self.n_cols, ctypes.byref(h))
        self.handle = h.value

    def matvec(self, d_z, d_out, stream=0):
        _call("zk_r1cs_matvec_device", self.handle, _ptr(d_z), _ptr(d_out), int(d_out.shape[0]), ctypes.c_void_p(stream))
        return d_out

    def matvec_transposed(self, d_x, d_out, x_len=None, stream=0):
        """d_out[j] = sum_i M[i][j] d_x[i] over the rows i < x_len (default: all of d_x); d_out[n_cols:] = 0.  The first call on a
        matrix builds its column-major companion on the device."""
        x_len = int(d_x.shape[0]) if x_len is None else int(x_len)
        _call("zk_r1cs_matvec_transposed_device", self.handle, _ptr(d_x), x_len, _ptr(d_out), int(d_out.shape[0]), ctypes.c_void_p(stream))
        return d_out

    def free(self):
        if self.handle:
            _call("zk_r1cs_matrix_free", self.handle)
            self.handle = 0


def witness_map(field, A, B, C, d_z, num_inputs, d_a, d_b, d_c, stream=0):
    """h = R1CStoQAP::witness_map(z) in HBM; d_a / d_b / d_c: device buffers of the domain size m (a power of two >=
    num_constraints + num_inputs); on return d_a holds the m coefficients of h (Montgomery), the last one zero"""
    m = int(d_a.shape[0])
    log_m = m.bit_length() - 1
    assert m == 1 << log_m and int(d_b.shape[0]) == m and int(d_c.shape[0]) == m
    _call("zk_groth16_witness_map_r1cs_device", field_id(field), A.handle, B.handle, C.handle, _ptr(d_z), num_inputs, log_m, _ptr(d_a), _ptr(d_b),
          _ptr(d_c), ctypes.c_void_p(stream))
    return d_a


R1CS_CHECK_SCRATCH_ELEMS = 256   # ZK_R1CS_CHECK_SCRATCH_ELEMS


def first_unsatisfied(A, B, C, d_z, stream=0):
    """ConstraintSystem::is_satisfied on the device, naming the row: the smallest i with <A_i, z> <B_i, z> != <C_i, z>, None when the
    assignment d_z (device buffer, canonical Montgomery) satisfies every row.  Synchronises the stream."""
    d_scratch = _new_buffer((3 * A.n_rows + R1CS_CHECK_SCRATCH_ELEMS, 4))
    row = ctypes.c_uint64(0)
    _call("zk_r1cs_first_unsatisfied_device", A.field, A.handle, B.handle, C.handle, _ptr(d_z), int(d_z.shape[0]), _ptr(d_scratch),
          int(d_scratch.shape[0]), ctypes.byref(row), ctypes.c_void_p(stream))
    return None if row.value == (1 << 64) - 1 else row.value


def assemble_proof(pairing, key_points, accs, r, s):
    """key_points: alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query0, b_g1_query0, b_g2_query0 (affine Montgomery limbs);
    accs: a_acc, b_g1_acc, l_acc, h_acc, b_g2_acc (Jacobian MSM results); r, s: Fr Montgomery limbs -> (A, B, C) affine"""
    pairing = ark_serialize.pairing_id(pairing)
    g1, g2 = ark_serialize.PAIRING_CURVES[pairing]
    keep = {k: _np64(v).ravel() for k, v in list(key_points.items()) + list(accs.items()) + [("r", r), ("s", s)]}
    asm = Assembly(**{k: ctypes.cast(_ptr(keep[k]), ctypes.c_void_p) for k, _ in Assembly._fields_})
    a, b, c = (np.zeros(2 * base_limbs(g1), dtype=np.uint64), np.zeros(2 * base_limbs(g2), dtype=np.uint64),
               np.zeros(2 * base_limbs(g1), dtype=np.uint64))
    _call("zk_groth16_assemble_proof", pairing, ctypes.byref(asm), _ptr(a), _ptr(b), _ptr(c))
    return a, b, c


class Prover:
    """One circuit: its proving key (query vectors resident as Bases, single elements on the host) and its R1CS matrices.
    `prove` is ark-groth16 0.3 create_proof from the full assignment on."""

    def __init__(self, pairing, pk, A, B, C, num_inputs, to_device):
        """pk: ark_serialize.ProvingKey (e.g. deserialize_unchecked of the file the reference's `compile` wrote)"""
        self.pairing = ark_serialize.pairing_id(pairing)
        self.field = "Bls381Fr" if self.pairing == ark_serialize.BLS12_381 else "Bn254Fr"
        self.A, self.B, self.C, self.num_inputs, self.to_device = A, B, C, num_inputs, to_device
        self.h_query, self.l_query = pk.upload("h_query"), pk.upload("l_query")
        self.a_query, self.b_g1_query, self.b_g2_query = (pk.upload("a_query", 1), pk.upload("b_g1_query", 1), pk.upload("b_g2_query", 1))
        self.points = {"alpha_g1": pk.points("alpha_g1")[0], "beta_g1": pk.points("beta_g1")[0], "delta_g1": pk.points("delta_g1")[0],
                       "beta_g2": pk.points("beta_g2")[0], "delta_g2": pk.points("delta_g2")[0], "a_query0": pk.points("a_query")[0],
                       "b_g1_query0": pk.points("b_g1_query")[0], "b_g2_query0": pk.points("b_g2_query")[0]}
        m = 1
        while m < A.n_rows + num_inputs:
            m *= 2
        self.m = m
        assert self.h_query.n == m - 1

    def prove(self, z_mont, r_mont, s_mont, stream=0):
        """z_mont: full assignment [num_vars, 4] Montgomery limbs, z[0] = 1 -> (A, B, C) affine points and the proof bytes"""
        return self.prove_device(self.to_device(_np64(z_mont)), r_mont, s_mont, stream=stream)

    def prove_device(self, d_z, r_mont, s_mont, stream=0):
        """`prove` from a resident assignment (e.g. encryption.EncryptCircuit.assign): no upload, and one device copy of d_z for the
        canonical form the MSMs read; d_z itself is left as it is"""
        ni, m = self.num_inputs, self.m
        d_abc = [_new_buffer((m, 4)) for _ in range(3)]                  # made on the device: the mat-vecs write all m entries
        d_h = witness_map(self.field, self.A, self.B, self.C, d_z, ni, d_abc[0], d_abc[1], d_abc[2], stream=stream)
        d_zc = d_z.copy() if isinstance(d_z, np.ndarray) else d_z.clone()
        vec_op(self.field, "into_repr", d_zc, stream=stream)             # the MSMs over z take canonical BigInts, like upstream
        # at most four MSMs in flight per device: submit four, collect one, submit the fifth.  The G2 MSM goes first: its host
        # tail (the Horner over the windows on Fq2 host limbs) is the longest of the five and then runs beside the G1 MSMs' device work
        t_b2 = msm_submit(self.b_g2_query, d_zc[1:], stream=stream, own_stream=True)
        t_h = msm_submit(self.h_query, d_h[:m - 1], montgomery=True, stream=stream, own_stream=True)
        t_l = msm_submit(self.l_query, d_zc[ni:], stream=stream, own_stream=True)
        t_a = msm_submit(self.a_query, d_zc[1:], stream=stream, own_stream=True)
        accs = {"b_g2_acc": t_b2.collect()}
        t_b1 = msm_submit(self.b_g1_query, d_zc[1:], stream=stream, own_stream=True)
        accs.update(h_acc=t_h.collect(), l_acc=t_l.collect(), a_acc=t_a.collect(), b_g1_acc=t_b1.collect())
        a, b, c = assemble_proof(self.pairing, self.points, accs, r_mont, s_mont)
        return (a, b, c), ark_serialize.proof_to_bytes(self.pairing, a, b, c)

    def free(self):
        for b in (self.h_query, self.l_query, self.a_query, self.b_g1_query, self.b_g2_query):
            b.free()
        for mtx in (self.A, self.B, self.C):
            mtx.free()


# ---- key generation: ark-groth16 0.3 generator.rs generate_parameters ----
def lagrange_coefficients(field, log_m, tau, d_out, stream=0):
    """d_out[i] = L_i(tau) on the size-2^log_m domain (evaluate_all_lagrange_coefficients); returns zt = tau^m - 1 (Montgomery limbs)"""
    zt = np.zeros(4, dtype=np.uint64)
    _call("zk_lagrange_coefficients_device", field_id(field), int(log_m), _ptr(_np64(tau)), _ptr(d_out), _ptr(zt), ctypes.c_void_p(stream))
    return zt


def qap_at(field, A, B, C, num_inputs, log_m, tau, d_u, d_v, d_w, stream=0):
    """LibsnarkReduction::instance_map_with_evaluation: the QAP polynomials u, v, w of every variable at tau (device buffers of
    n_vars elements); returns zt"""
    zt = np.zeros(4, dtype=np.uint64)
    n_vars = int(d_u.shape[0])
    assert int(d_v.shape[0]) == n_vars and int(d_w.shape[0]) == n_vars
    _call("zk_groth16_qap_at_device", field_id(field), A.handle, B.handle, C.handle, int(num_inputs), int(log_m), _ptr(_np64(tau)), _ptr(d_u),
          _ptr(d_v), _ptr(d_w), n_vars, _ptr(zt), ctypes.c_void_p(stream))
    return zt


def key_scalars(field, d_u, d_v, d_w, num_inputs, log_m, alpha, beta, gamma, delta, tau, zt, d_abc, d_h, stream=0):
    """d_abc = (beta u + alpha v + w) / gamma for the inputs, / delta for the rest; d_h[i] = tau^i zt / delta, i < 2^log_m - 1"""
    sc = [_np64(x) for x in (alpha, beta, gamma, delta, tau, zt)]
    _call("zk_groth16_key_scalars_device", field_id(field), _ptr(d_u), _ptr(d_v), _ptr(d_w), int(d_u.shape[0]), int(num_inputs), int(log_m),
          *[_ptr(x) for x in sc], _ptr(d_abc), _ptr(d_h) if int(d_h.shape[0]) else None, ctypes.c_void_p(stream))
    return d_abc, d_h


def _on_emulator():
    return backend_info().startswith("emu")


def _new_buffer(shape):
    """zero device buffer of u64 limbs: a torch tensor on the GPU (numpy under the CPU test emulator, whose device memory is host memory)"""
    if _on_emulator():
        return np.zeros(shape, dtype=np.uint64)
    import torch
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def _upload(arr):
    arr = _np64(arr)
    if _on_emulator():
        return arr.copy()
    import torch
    return torch.from_numpy(arr.view(np.int64)).cuda()


def _download(buf):
    if isinstance(buf, np.ndarray):
        return buf
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint64)


def _synchronize():
    if not _on_emulator():
        import torch
        torch.cuda.synchronize()


class Parameters:
    """ark-groth16 0.3 ProvingKey<E> as generate_parameters leaves it, the point vectors resident on the device.  Offers what
    `Prover` asks of a key (`points`, `upload`, `count`), so a prover can be built from it without a round trip through bytes."""

    def __init__(self, pairing, num_inputs, device_members):
        self.pairing, self.num_inputs, self.device = ark_serialize.pairing_id(pairing), num_inputs, device_members
        self._host = {}

    def _curve(self, name):
        return ark_serialize.PAIRING_CURVES[self.pairing][1 if name in ark_serialize.G2_MEMBERS else 0]

    def count(self, name):
        return int(self.device[name].shape[0])

    def points(self, name):
        """member `name` as host limbs [count, 2 * limbs] (copied from the device once)"""
        if name not in self._host:
            self._host[name] = np.ascontiguousarray(_download(self.device[name])).reshape(self.count(name), -1)
        return self._host[name]

    def upload(self, name, skip_first=0):
        """-> Bases over the resident member (zk_bases_adopt_device: no copy); skip_first as ProvingKey.upload"""
        return Bases(self._curve(name), device_tensor=self.device[name][skip_first:], n=self.count(name) - skip_first)

    def members(self):
        return {name: self.points(name) for name in ark_serialize.PK_MEMBERS}

    def serialize_unchecked(self):
        """the bytes of ProvingKey::serialize_unchecked: the key file the reference's `compile` writes (lib/src/utils.rs:85-102)"""
        return ark_serialize.ProvingKey.serialize_unchecked(self.pairing, self.members())

    def verifying_key_bytes(self):
        """ark_to_bytes(pk.vk): compressed"""
        return ark_serialize.verifying_key_to_bytes(self.pairing, {name: self.points(name) for name in ark_serialize.VK_MEMBERS})


def generate_parameters(pairing, A, B, C, num_inputs, n_vars, alpha, beta, gamma, delta, tau, g1=None, g2=None, stream=0):
    """ark-groth16 0.3 generate_parameters from the resident R1CS matrices (A, B, C: R1csMatrix) and a given trapdoor (Montgomery
    limbs).  g1 / g2: the group generators as affine Montgomery points, None = the curves' standard generators (upstream draws
    random ones).  All per-element work runs on the device, on `stream`; returns Parameters once it has finished."""
    pairing = ark_serialize.pairing_id(pairing)
    field = "Bls381Fr" if pairing == ark_serialize.BLS12_381 else "Bn254Fr"
    c1, c2 = ark_serialize.PAIRING_CURVES[pairing]
    m, log_m = 1, 0
    while m < A.n_rows + num_inputs:
        m, log_m = 2 * m, log_m + 1
    d_u, d_v, d_w = (_new_buffer((n_vars, 4)) for _ in range(3))
    zt = qap_at(field, A, B, C, num_inputs, log_m, tau, d_u, d_v, d_w, stream=stream)
    d_h = _new_buffer((m - 1, 4))
    key_scalars(field, d_u, d_v, d_w, num_inputs, log_m, alpha, beta, gamma, delta, tau, zt, d_w, d_h, stream=stream)   # abc over w
    d_s1, d_s2 = _upload(np.stack([_np64(alpha), _np64(beta), _np64(delta)])), _upload(np.stack([_np64(beta), _np64(gamma), _np64(delta)]))
    l1, l2 = 2 * base_limbs(c1), 2 * base_limbs(c2)

    def fixed_base(curve, base, d_scalars, limbs):
        out = _new_buffer((int(d_scalars.shape[0]), limbs))
        fixed_base_msm_device(curve, d_scalars, out, int(d_scalars.shape[0]), base=base, montgomery=True, stream=stream)
        return out

    p_s1, p_s2 = fixed_base(c1, g1, d_s1, l1), fixed_base(c2, g2, d_s2, l2)
    p_a, p_b1, p_b2 = fixed_base(c1, g1, d_u, l1), fixed_base(c1, g1, d_v, l1), fixed_base(c2, g2, d_v, l2)
    p_h, p_abc = fixed_base(c1, g1, d_h, l1), fixed_base(c1, g1, d_w, l1)
    _synchronize()      # the scalar buffers go out of scope here
    return Parameters(pairing, num_inputs, {
        "alpha_g1": p_s1[0:1], "beta_g1": p_s1[1:2], "delta_g1": p_s1[2:3], "beta_g2": p_s2[0:1], "gamma_g2": p_s2[1:2], "delta_g2": p_s2[2:3],
        "gamma_abc_g1": p_abc[:num_inputs], "l_query": p_abc[num_inputs:], "a_query": p_a, "b_g1_query": p_b1, "b_g2_query": p_b2,
        "h_query": p_h})


def generate_random_parameters(pairing, A, B, C, num_inputs, n_vars, g1=None, g2=None, stream=0):
    """generate_random_parameters: alpha, beta, gamma, delta, tau from the operating system's generator (`secrets`), nonzero, tau
    outside the evaluation domain (upstream: sample_element_outside_domain)"""
    pairing = ark_serialize.pairing_id(pairing)
    field = "Bls381Fr" if pairing == ark_serialize.BLS12_381 else "Bn254Fr"
    p = field_modulus(field)
    m = 1
    while m < A.n_rows + num_inputs:
        m *= 2
    draw = lambda: 1 + secrets.randbelow(p - 1)
    tau = draw()
    while pow(tau, m, p) == 1:
        tau = draw()
    ints = [draw() for _ in range(4)] + [tau]
    mont = ark_serialize.scalars_from_bytes(field, b"".join(v.to_bytes(32, "little") for v in ints), 5)
    return generate_parameters(pairing, A, B, C, num_inputs, n_vars, mont[0], mont[1], mont[2], mont[3], mont[4], g1=g1, g2=g2, stream=stream)


# ---- verification: ark-groth16 0.3 verifier.rs ----
class MalformedVerifyingKey(ValueError):
    """SynthesisError::MalformedVerifyingKey: len(public_inputs) + 1 != len(gamma_abc_g1)"""


def pairing_product(pairing, g1_points, g2_points):
    """final_exponentiation(prod_i miller_loop(g1[i], g2[i])) -> the 12 Fq coefficients (Montgomery limbs) in ark's Fp12 order,
    [12, limbs]; the points must be in their r-order subgroups; (0, 0) in either slot contributes 1"""
    pairing = ark_serialize.pairing_id(pairing)
    c1, c2 = ark_serialize.PAIRING_CURVES[pairing]
    a, b = _np64(g1_points).reshape(-1, 2 * base_limbs(c1)), _np64(g2_points).reshape(-1, 2 * base_limbs(c2))
    assert a.shape[0] == b.shape[0]
    out = np.zeros((12, base_limbs(c1)), dtype=np.uint64)
    _call("zk_pairing_product", pairing, _ptr(a), _ptr(b), a.shape[0], _ptr(out))
    return out


class VerifyingKey:
    """ark-groth16 0.3 VerifyingKey<E>: alpha_g1, beta_g2, gamma_g2, delta_g2 as host limbs, gamma_abc_g1 resident on the device
    ([len, 2 * limbs] u64) with a `Bases` handle over gamma_abc_g1[1..] for prepare_inputs."""

    def __init__(self, pairing, alpha_g1, beta_g2, gamma_g2, delta_g2, d_gamma_abc_g1):
        self.pairing = ark_serialize.pairing_id(pairing)
        self.g1, self.g2 = ark_serialize.PAIRING_CURVES[self.pairing]
        self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2 = (_np64(x).ravel().copy() for x in (alpha_g1, beta_g2, gamma_g2, delta_g2))
        self.d_gamma_abc_g1 = d_gamma_abc_g1
        self.n = int(d_gamma_abc_g1.shape[0])
        if self.n == 0:
            raise MalformedVerifyingKey("gamma_abc_g1 is empty")
        self.gamma_abc0 = np.ascontiguousarray(_download(d_gamma_abc_g1[0:1])).ravel().copy()
        self.tail = Bases(self.g1, device_tensor=d_gamma_abc_g1[1:], n=self.n - 1) if self.n > 1 else None

    @classmethod
    def deserialize(cls, pairing, buf, stream=0):
        """CanonicalDeserialize::deserialize of the reference's verifying-key file (lib/src/utils.rs:112-118; compressed):
        every point is checked (canonical, flags, on the curve, in the subgroup) -- the three G2 members and alpha_g1 by the
        host decoder, gamma_abc_g1 by the device decoder, whose output stays resident.  Raises ark_serialize.PointDecodeError."""
        pairing = ark_serialize.pairing_id(pairing)
        buf = bytes(buf)
        g1, g2 = ark_serialize.PAIRING_CURVES[pairing]
        s1, s2 = ark_serialize.point_size(g1, True), ark_serialize.point_size(g2, True)
        head = s1 + 3 * s2
        if len(buf) < head + 8:
            raise ValueError("truncated verifying key")
        n = int.from_bytes(buf[head:head + 8], "little")
        if len(buf) != head + 8 + n * s1:
            raise ValueError("the verifying key's length does not match its gamma_abc_g1 count")
        alpha = ark_serialize.points_from_bytes_checked(g1, buf[:s1], 1)
        g2s = ark_serialize.points_from_bytes_checked(g2, buf[s1:head], 3)
        d_abc = _new_buffer((n, 2 * base_limbs(g1)))
        ark_serialize.points_from_bytes_checked_device(g1, buf[head + 8:], n, d_abc, compressed=True, stream=stream)
        return cls(pairing, alpha[0], g2s[0], g2s[1], g2s[2], d_abc)

    @classmethod
    def from_parameters(cls, params):
        """pk.vk of a `Parameters`: gamma_abc_g1 is adopted where generate_parameters left it"""
        return cls(params.pairing, params.points("alpha_g1")[0], params.points("beta_g2")[0], params.points("gamma_g2")[0],
                   params.points("delta_g2")[0], params.device["gamma_abc_g1"])

    def free(self):
        if self.tail is not None:
            self.tail.free()
            self.tail = None


class PreparedVerifyingKey:
    """ark-groth16 0.3 PreparedVerifyingKey: the key and the cached e(alpha_g1, beta_g2) (the negated G2 members are formed inside
    zk_groth16_verify)"""

    def __init__(self, vk, alpha_g1_beta_g2):
        self.vk, self.alpha_g1_beta_g2 = vk, alpha_g1_beta_g2


def prepare_verifying_key(vk):
    return PreparedVerifyingKey(vk, pairing_product(vk.pairing, vk.alpha_g1, vk.beta_g2))


def prepare_inputs(pvk, public_inputs, stream=0):
    """g_ic = gamma_abc_g1[0] + sum_i x_i gamma_abc_g1[i + 1] as an affine point (host limbs).  public_inputs: Fr elements in
    Montgomery form, [l, 4] -- host limbs (uploaded) or a device buffer.  One MSM over the resident gamma_abc_g1[1..]; a length
    mismatch raises MalformedVerifyingKey and launches nothing."""
    vk = pvk.vk
    d_x = _upload(np.asarray(public_inputs, dtype=np.uint64).reshape(-1, 4)) if isinstance(public_inputs, (np.ndarray, list, tuple)) else public_inputs
    n_in = int(d_x.shape[0])
    if n_in + 1 != vk.n:
        raise MalformedVerifyingKey("%d public inputs for a key with %d gamma_abc_g1 points" % (n_in, vk.n))
    out = np.zeros(2 * base_limbs(vk.g1), dtype=np.uint64)
    _call("zk_groth16_prepare_inputs", curve_id(vk.g1), vk.tail.handle if vk.tail is not None else 0, _ptr(vk.gamma_abc0), vk.n,
          _ptr(d_x) if n_in else None, n_in, _ptr(out), ctypes.c_void_p(stream))
    return out


def verify_proof_with_prepared_inputs(pvk, proof, g_ic):
    """e(A, B) e(g_ic, -gamma_g2) e(C, -delta_g2) == e(alpha_g1, beta_g2); proof = (A, B, C) affine limbs -> bool"""
    vk = pvk.vk
    a, b, c = (_np64(x).ravel() for x in proof)
    g_ic = _np64(g_ic).ravel()
    pts = VkPoints(*[ctypes.cast(_ptr(x), ctypes.c_void_p) for x in (vk.alpha_g1, vk.beta_g2, vk.gamma_g2, vk.delta_g2)])
    ab = _np64(pvk.alpha_g1_beta_g2)
    ok = ctypes.c_uint64(0)
    _call("zk_groth16_verify", vk.pairing, ctypes.byref(pts), _ptr(ab), _ptr(g_ic), _ptr(a), _ptr(b), _ptr(c), ctypes.byref(ok))
    return bool(ok.value)


def verify(vk, public_inputs, proof, stream=0):
    """Groth16::verify: vk a VerifyingKey (or a PreparedVerifyingKey, to reuse its cached pairing); proof = (A, B, C) affine limbs or
    the 192 / 128 bytes of ark_to_bytes(proof), which go through the checked host decoder -> bool"""
    pvk = vk if isinstance(vk, PreparedVerifyingKey) else prepare_verifying_key(vk)
    if isinstance(proof, (bytes, bytearray, memoryview)):
        proof = ark_serialize.proof_from_bytes_checked(pvk.vk.pairing, bytes(proof))
    return verify_proof_with_prepared_inputs(pvk, proof, prepare_inputs(pvk, public_inputs, stream=stream))
