"""Mirror of circuits-ark/src/encryption.rs: the ElGamal-over-JubJub encryption of the reference's `sell` / `buy` path and the
circuit Groth16 proves about it ("EncryptCircuit").

  Parameters(n, poseidon)               Parameters<C>
  keygen / encrypt / decrypt            EncryptCircuit::{keygen, encrypt, decrypt}; the c2 stream stays on the device
  get_public_inputs                     [c1.x, c1.y] + c2 padded with zeros to n (encryption.rs:139-152), a device buffer
  bytes_to_plaintext_chunks_direct      utils.rs:60-72 on the device
  EncryptCircuit.csr / matrices         the R1CS of generate_constraints (own layout), host CSR / resident R1csMatrix
  EncryptCircuit.assign                 the full assignment as a device buffer: the fixed section from the host, the four per-element
                                        segments from one kernel (zk_encrypt_witness_device); z never visits the host

Assignment layout, with F fixed witnesses and num_inputs = n + 3:

  z = [1 | c1.x c1.y | c2[0..n) | fixed (F) | m[0..n) | b[0..n) | k[0..n)]

Rows: the fixed section first, then four per element i, with dh the last fixed witness:

  b_i (1 - b_i) = 0      c2_i k_i = b_i      c2_i (1 - b_i) = 0      (m_i + dh - c2_i) b_i = 0

Upstream's quirk is kept: a ciphertext element equal to 0 counts as empty (b_i = 0) and leaves its plaintext unconstrained.
The randomness r and the Groth16 blinds are arguments, as everywhere in this library."""
import ctypes

import numpy as np

from . import _call, _ptr, field_id, i32, jubjub, load, poseidon, r1cs, u64, vp
from .groth16 import R1csMatrix, _new_buffer, _on_emulator, _upload

SIGNATURES = {
    "zk_encrypt_witness_device": [i32, vp, u64, u64, vp, vp, vp, vp, vp, vp],
    "zk_plaintext_from_bytes_device": [i32, vp, u64, vp, u64, vp],
}
PROVER_EXPORTS = list(SIGNATURES)
_elib = load        # the bound handle (tests and tools take it for raw calls)

FIELD = "Bls381Fr"
_MASK64 = (1 << 64) - 1


class Parameters:
    """Parameters<C>: n, the length every plaintext and ciphertext is padded to, and the Poseidon parameter set of the mask"""

    def __init__(self, n, poseidon):
        self.n, self.poseidon = int(n), poseidon
        if self.n < 1 or poseidon.field != field_id(FIELD) or poseidon.rate_offset + 2 > poseidon.width:
            raise ValueError("Parameters: n >= 1 and a Poseidon set over %s with two rate slots" % FIELD)


def keygen(sk, base=None):
    return jubjub.keygen(sk, base)


def shared_digest(point, params):
    """dh = the sponge hash of the shared point's affine (x, y), on the library's host twin"""
    return params.poseidon.hash([point[0], point[1]])


def encrypt(pk, msg_dev, r, params, base=None, stream=0):
    """-> (c1, c2_dev): c1 = [r] G as affine integers, c2[i] = msg[i] + dh over the device buffer msg_dev (at most n elements)"""
    if int(msg_dev.shape[0]) > params.n:
        raise ValueError("encrypt: the message has more than n = %d elements" % params.n)
    c1 = jubjub.mul(r, jubjub.GENERATOR if base is None else base)
    dh = shared_digest(jubjub.mul(r, pk), params)
    return c1, poseidon.elgamal_mask(FIELD, msg_dev, dh, stream=stream)


def decrypt(cipher, sk, params, stream=0):
    """-> the plaintext as a device buffer: c2[i] - H([sk] c1)"""
    c1, c2_dev = cipher
    dh = shared_digest(jubjub.mul(sk, c1), params)
    return poseidon.elgamal_unmask(FIELD, c2_dev, dh, stream=stream)


def get_public_inputs(cipher, params):
    """-> device buffer [n + 2, 4]: c1.x, c1.y, then c2 padded with zeros to n"""
    c1, c2_dev = cipher
    have = int(c2_dev.shape[0])
    if have > params.n:
        raise ValueError("get_public_inputs: the ciphertext has more than n = %d elements" % params.n)
    out = _new_buffer((params.n + 2, 4))
    out[0:2] = _upload(poseidon.to_mont(jubjub.P, [c1[0], c1[1]]))
    out[2:2 + have] = c2_dev
    return out


def bytes_to_plaintext_chunks_direct(data, size, stream=0):
    """-> device buffer [size, 4]: element i = byte i of `data`, zero from len(data) on; bytes from `size` on are dropped"""
    data = bytes(data)[:size]
    out = _new_buffer((size, 4))
    if data:
        host = np.frombuffer(data, dtype=np.uint8).copy()
        if _on_emulator():
            d_bytes = host
        else:
            import torch
            d_bytes = torch.from_numpy(host).cuda()
    else:
        d_bytes = None
    _call("zk_plaintext_from_bytes_device", field_id(FIELD), _ptr(d_bytes) if d_bytes is not None else None, len(data), _ptr(out), int(size),
          ctypes.c_void_p(stream))
    if d_bytes is not None and not _on_emulator():
        import torch
        torch.cuda.synchronize()        # d_bytes goes out of scope here
    return out


def encrypt_witness(msg_dev, msg_len, n, dh, c2_dev, m_dev, b_dev, k_dev, stream=0):
    """zk_encrypt_witness_device over Bls381Fr: the four per-element segments from the plaintext and dh (an integer)"""
    s = poseidon.to_mont(jubjub.P, [dh])
    _call("zk_encrypt_witness_device", field_id(FIELD), _ptr(msg_dev) if msg_len else None, int(msg_len), int(n), _ptr(s), _ptr(c2_dev), _ptr(m_dev),
          _ptr(b_dev), _ptr(k_dev), ctypes.c_void_p(stream))


class EncryptCircuit:
    """The statement of encryption.rs:219-263: there are r, pk and m with c1 = [r] base and, for every ciphertext element that is not
    zero, c2_i = m_i + H([r] pk).  scalar_bits: the bits of r the circuit allocates -- 256 is upstream's to_bytes![r]; a smaller value
    needs r < 2^scalar_bits and exists so that a whole proof fits the CPU test tier.  The matrices depend on (n, scalar_bits, the
    Poseidon set, base) alone."""

    def __init__(self, params, base=jubjub.GENERATOR, scalar_bits=256):
        if jubjub.A != jubjub.P - 1 or not jubjub.is_on_curve(base) or scalar_bits < 1:
            raise ValueError("EncryptCircuit: the base point is not on the curve")
        self.params, self.base, self.scalar_bits = params, (int(base[0]), int(base[1])), int(scalar_bits)
        self.n = params.n
        self.num_inputs = self.n + 3
        self._layout = self.fixed_section(None, None, None)                # the fixed rows, laid out once without values
        self.num_fixed, self.num_fixed_rows = self._layout.num_witnesses, len(self._layout.rows)
        self.n_vars = self.num_inputs + self.num_fixed + 3 * self.n
        self.m0 = self.num_inputs + self.num_fixed                  # columns of m, b, k and of dh (the last fixed witness)
        self.b0, self.k0, self.dh_col = self.m0 + self.n, self.m0 + 2 * self.n, self.m0 - 1
        self._csr = None

    def _column(self, var):
        """fixed-section variable -> column of z: the constant one, c1.x, c1.y in place; witness j behind the n + 3 inputs"""
        return var if var >= 0 else self.num_inputs - 1 - var

    def fixed_section(self, pk, r, c1):
        """the fixed section on a fresh builder: rows, and values when pk, r, c1 are given.  Order of allocation: the bits of r, pk,
        s = [r] pk, c1' = [r] base, dh = H(s), c1' == c1."""
        cs = r1cs.ConstraintSystem(jubjub.P)
        known = pk is not None
        c1x, c1y = cs.new_input(c1[0] if known else None), cs.new_input(c1[1] if known else None)
        bits = [r1cs.boolean(cs, (r >> i) & 1 if known else None) for i in range(self.scalar_bits)]
        pkv = ({cs.new_witness(pk[0] if known else None): 1}, {cs.new_witness(pk[1] if known else None): 1})
        r1cs.on_curve(cs, jubjub.D, pkv)
        s = r1cs.scalar_mul_le(cs, jubjub.D, bits, pkv)
        c1v = r1cs.scalar_mul_le(cs, jubjub.D, bits, self.base)
        r1cs.poseidon_hash(cs, self.params.poseidon, [s[0], s[1]])
        cs.enforce(c1v[0], {r1cs.ONE: 1}, {c1x: 1})
        cs.enforce(c1v[1], {r1cs.ONE: 1}, {c1y: 1})
        return cs

    def num_constraints(self):
        return self.num_fixed_rows + 4 * self.n

    def csr(self):
        """-> [(row_ptr u64, col u32, val u64 [nnz, 4]) for A, B, C]: host numpy, no device.  n_cols = self.n_vars."""
        if self._csr is not None:
            return self._csr
        p, n = jubjub.P, self.n
        memo = {}

        def mont(c):
            if c not in memo:
                v = (c << 256) % p
                memo[c] = [(v >> (64 * k)) & _MASK64 for k in range(4)]
            return memo[c]

        cs = self._layout
        i = np.arange(n, dtype=np.int64)
        c2, m, b, k = 3 + i, self.m0 + i, self.b0 + i, self.k0 + i
        dh, one = np.full(n, self.dh_col, dtype=np.int64), np.zeros(n, dtype=np.int64)
        plus, minus = np.array(mont(1), dtype=np.uint64), np.array(mont(p - 1), dtype=np.uint64)
        # per element, rows 1 .. 4: (columns, signs, terms per row) of each side
        sides = [([b, c2, c2, m, dh, c2], [1, 1, 1, 1, 1, -1], [1, 1, 1, 3]),
                 ([one, b, k, one, b, b], [1, -1, 1, 1, -1, 1], [2, 1, 2, 1]),
                 ([b], [1], [0, 1, 0, 0])]
        out = []
        for (f_ptr, f_cols, f_vals), (cols, signs, lens) in zip(cs.csr(self._column, mont), sides):
            e_cols = np.stack(cols, axis=1).ravel()
            e_vals = np.tile(np.stack([plus if s > 0 else minus for s in signs]), (n, 1))
            starts = np.concatenate([[0], np.cumsum(lens)])                                  # offsets of an element's four rows, and its total
            e_ptr = (i[:, None] * int(starts[-1]) + starts[None, 1:]).ravel() + f_ptr[-1]
            out.append((np.concatenate([np.array(f_ptr, dtype=np.uint64), e_ptr.astype(np.uint64)]),
                        np.concatenate([np.array(f_cols, dtype=np.uint32), e_cols.astype(np.uint32)]),
                        np.concatenate([np.array(f_vals, dtype=np.uint64).reshape(-1, 4), e_vals])))
        self._csr = out
        return out

    def matrices(self):
        """-> (A, B, C) as resident groth16.R1csMatrix"""
        return tuple(R1csMatrix(FIELD, csr=side, n_cols=self.n_vars) for side in self.csr())

    def fixed_assignment(self, pk, r):
        """the host's share of z: (c1, dh, [1, c1.x, c1.y], the F fixed witnesses) as integers"""
        r = int(r)
        if not 0 <= r < 1 << self.scalar_bits:
            raise ValueError("assign: r does not fit %d bits" % self.scalar_bits)
        if not jubjub.is_on_curve(pk):
            raise ValueError("assign: pk is not on the curve")
        c1 = jubjub.mul(r, self.base)
        cs = self.fixed_section(pk, r, c1)
        return c1, cs.witness_values[-1], [1, c1[0], c1[1]], cs.witness_values

    def assign(self, pk, r, msg_dev, msg_len=None, stream=0):
        """-> d_z, the full assignment [n_vars, 4] on the device.  The host computes the fixed section and uploads it once; one kernel
        fills c2, m, b, k from msg_dev[:msg_len] (default: all of msg_dev)."""
        n = self.n
        msg_len = int(msg_dev.shape[0]) if msg_len is None else int(msg_len)
        if msg_len > n or msg_len > int(msg_dev.shape[0]):
            raise ValueError("assign: msg_len = %d exceeds n = %d or the message buffer" % (msg_len, n))
        _, dh, head, fixed = self.fixed_assignment(pk, r)
        d_z = _new_buffer((self.n_vars, 4))
        d_host = _upload(poseidon.to_mont(jubjub.P, head + fixed))
        d_z[0:3] = d_host[0:3]
        d_z[self.num_inputs:self.m0] = d_host[3:]
        encrypt_witness(msg_dev, msg_len, n, dh, d_z[3:3 + n], d_z[self.m0:self.b0], d_z[self.b0:self.k0], d_z[self.k0:], stream=stream)
        return d_z
