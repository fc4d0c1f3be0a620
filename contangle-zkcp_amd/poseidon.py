"""Poseidon, the Merkle tree over it and the ElGamal c2 stream: mirrors of the upstream names the reference's seller path uses
outside Groth16::prove ("Poseidon"; the semantics are restated there, parity status "unpinned").

  ark_sponge::poseidon::{PoseidonParameters, PoseidonSponge}     <- ark-sponge 0.3 (rate 2, capacity 1, capacity element first)
  ark_crypto_primitives::crh::poseidon::{CRH, TwoToOneCRH}       <- one input on the host twin, *_batch on device buffers
  ark_crypto_primitives::merkle_tree::{MerkleTree, Path}         <- MerkleTree::new on the device; Path::verify on the host twin
  EncryptCircuit::encrypt / decrypt's c2 stream                  <- elgamal_mask / elgamal_unmask

Field elements cross this interface as Python integers (canonical); device buffers hold Montgomery limbs [.., 4] like every other
vector of the library.  The library hard-codes no parameter set."""
import ctypes

import numpy as np

from . import ZK_ERR_INVALID_ARG, ZkError, _call, _check, _np64, _ptr, field_id, field_modulus, i32, load, ptr, u32, u64, vp

_MASK64 = (1 << 64) - 1


SIGNATURES = {
    "zk_poseidon_create": [i32, u32, u32, u32, u32, u32, u64, vp, vp, vp, ptr(u64)],
    "zk_poseidon_free": [u64],
    "zk_poseidon_permute_host": [u64, vp, u64],
    "zk_poseidon_hash_host": [u64, vp, u32, u64, vp],
    "zk_poseidon_permute_device": [u64, vp, u64, vp],
    "zk_poseidon_hash_device": [u64, vp, u32, u64, vp, vp],
    "zk_poseidon_merkle_tree_device": [u64, vp, u32, u32, vp, vp],
    "zk_merkle_paths_device": [i32, vp, u32, vp, u64, vp, vp],
    "zk_vec_add_scalar_device": [i32, vp, vp, u64, vp, vp],
}
PROVER_EXPORTS = list(SIGNATURES)
_plib = load        # the bound handle (tests and tools take it for raw calls)


def _bind(lib):
    """kept for callers that hold a handle of load(): it is bound already"""
    return lib


def to_mont(p, values):
    """Python integers (taken mod p) -> Montgomery limbs, uint64 [len, 4]"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, x in enumerate(values):
        v = ((int(x) % p) << 256) % p
        out[i] = [(v >> (64 * k)) & _MASK64 for k in range(4)]
    return out


def from_mont(p, limbs):
    """Montgomery limbs [.., 4] -> the canonical Python integers, flat"""
    rinv = pow(1 << 256, -1, p)
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) * rinv % p for row in _np64(limbs).reshape(-1, 4).tolist()]


class PoseidonParameters:
    """ark_sponge::poseidon::PoseidonParameters::new(full_rounds, partial_rounds, alpha, mds, ark) plus the two things ark-sponge 0.3
    hard-codes: the rate (2) and where the capacity sits (first).  capacity_first=False with init=[0, 0, L << 64] is
    halo2_gadgets' ConstantLength<L> at width 3.  mds: width x width, ark: (full_rounds + partial_rounds) x width, integers (taken
    mod p, as ark-ff 0.3 from_str does with the reference's over-long decimal constants)."""

    def __init__(self, field, full_rounds, partial_rounds, alpha, mds, ark, rate=2, capacity_first=True, init=None):
        self.field = field_id(field)
        self.p = field_modulus(self.field)
        self.width = len(mds)
        self.rate, self.capacity = int(rate), self.width - int(rate)
        self.rate_offset = self.capacity if capacity_first else 0
        self.full_rounds, self.partial_rounds, self.alpha = int(full_rounds), int(partial_rounds), int(alpha)
        if any(len(row) != self.width for row in mds) or len(ark) != self.full_rounds + self.partial_rounds or \
                any(len(row) != self.width for row in ark) or (init is not None and len(init) != self.width) or not 0 <= self.alpha <= _MASK64:
            raise ValueError("PoseidonParameters: mds, ark, init and alpha do not fit the stated shape")
        ark_m = to_mont(self.p, [x for row in ark for x in row])
        mds_m = to_mont(self.p, [x for row in mds for x in row])
        init_m = to_mont(self.p, init) if init is not None else None
        h = ctypes.c_uint64(0)
        self._lib = _plib()       # a handle belongs to the library instance that made it
        _check(self._lib.zk_poseidon_create(self.field, self.width, max(self.rate, 0), max(self.rate_offset, 0), self.full_rounds, self.partial_rounds,
                                          self.alpha, _ptr(ark_m), _ptr(mds_m), _ptr(init_m) if init_m is not None else None, ctypes.byref(h)),
               "zk_poseidon_create")
        self.handle = h.value
        self.init = [int(x) % self.p for x in init] if init is not None else [0] * self.width
        # the constants as integers: the R1CS gadget (r1cs.poseidon_permute) writes them into its rows
        self.ark = [[int(x) % self.p for x in row] for row in ark]
        self.mds = [[int(x) % self.p for x in row] for row in mds]

    def permute(self, state):
        """one permutation of `width` integers on the host twin"""
        s = to_mont(self.p, state)
        if len(state) != self.width:
            raise ValueError("permute: the state has %d elements, the width is %d" % (len(state), self.width))
        _check(self._lib.zk_poseidon_permute_host(self.handle, _ptr(s), 1), "zk_poseidon_permute_host")
        return from_mont(self.p, s)

    def hash(self, elems):
        """the sponge hash of a non-empty list of integers on the host twin"""
        x = to_mont(self.p, elems)
        out = np.zeros((1, 4), dtype=np.uint64)
        _check(self._lib.zk_poseidon_hash_host(self.handle, _ptr(x), len(elems), 1, _ptr(out)), "zk_poseidon_hash_host")
        return from_mont(self.p, out)[0]

    def hash_batch(self, in_dev, arity, out=None, stream=0):
        """zk_poseidon_hash_device: in_dev holds count x arity elements; returns the count digests (device buffer)"""
        from .groth16 import _new_buffer
        total = int(np.prod(in_dev.shape[:-1]))
        if arity < 1 or total % arity:
            raise ZkError(ZK_ERR_INVALID_ARG, "hash_batch: %d elements are no multiple of the arity %d" % (total, arity))
        count = total // arity
        if out is None:
            out = _new_buffer((count, 4))
        _check(self._lib.zk_poseidon_hash_device(self.handle, _ptr(in_dev), arity, count, _ptr(out), ctypes.c_void_p(stream)), "zk_poseidon_hash_device")
        return out

    def permute_batch(self, states_dev, stream=0):
        """zk_poseidon_permute_device: count states of `width` elements, in place"""
        total = int(np.prod(states_dev.shape[:-1]))
        if total % self.width:
            raise ZkError(ZK_ERR_INVALID_ARG, "permute_batch: %d elements are no multiple of the width %d" % (total, self.width))
        _check(self._lib.zk_poseidon_permute_device(self.handle, _ptr(states_dev), total // self.width, ctypes.c_void_p(stream)),
               "zk_poseidon_permute_device")
        return states_dev

    def free(self):
        if self.handle:
            _check(self._lib.zk_poseidon_free(self.handle), "zk_poseidon_free")
            self.handle = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PoseidonSponge:
    """ark-sponge 0.3 PoseidonSponge (CryptographicSponge::absorb / squeeze_field_elements over one field): the duplex bookkeeping
    in Python, every permutation on the host twin."""

    def __init__(self, params):
        self.params = params
        self.state = list(params.init)
        self.mode, self.index = "absorbing", 0

    def _permute(self):
        self.state = self.params.permute(self.state)

    def absorb(self, elems):
        elems = [int(x) % self.params.p for x in (elems if isinstance(elems, (list, tuple)) else [elems])]
        if not elems:
            return
        pr, r, off = self.params, self.params.rate, self.params.rate_offset
        if self.mode == "squeezing":
            self._permute()
            start = 0
        else:
            start = self.index
            if start == r:
                self._permute()
                start = 0
        while True:
            if start + len(elems) <= r:
                for i, x in enumerate(elems):
                    self.state[off + start + i] = (self.state[off + start + i] + x) % pr.p
                self.mode, self.index = "absorbing", start + len(elems)
                return
            take = r - start
            for i, x in enumerate(elems[:take]):
                self.state[off + start + i] = (self.state[off + start + i] + x) % pr.p
            self._permute()
            elems, start = elems[take:], 0

    def squeeze_field_elements(self, count):
        r, off = self.params.rate, self.params.rate_offset
        if self.mode == "absorbing":
            self._permute()
            start = 0
        else:
            start = self.index
            if start == r:
                self._permute()
                start = 0
        out = []
        while True:
            if start + (count - len(out)) <= r:
                need = count - len(out)
                out += self.state[off + start:off + start + need]
                self.mode, self.index = "squeezing", start + need
                return out
            out += self.state[off + start:off + r]
            self._permute()
            start = 0


class CRH:
    """ark_crypto_primitives::crh::poseidon::CRH: evaluate(params, input) = absorb the input, squeeze one element"""

    @staticmethod
    def evaluate(params, elems):
        return params.hash(list(elems))

    @staticmethod
    def evaluate_batch(params, in_dev, arity, out=None, stream=0):
        return params.hash_batch(in_dev, arity, out, stream)


class TwoToOneCRH:
    """...::TwoToOneCRH: evaluate / compress(params, left, right) = the hash of [left, right]"""

    @staticmethod
    def evaluate(params, left, right):
        return params.hash([left, right])

    compress = evaluate

    @staticmethod
    def evaluate_batch(params, pairs_dev, out=None, stream=0):
        """pairs_dev: [count, 2, 4] (left, right) -> [count, 4]"""
        return params.hash_batch(pairs_dev, 2, out, stream)

    compress_batch = evaluate_batch


class Path:
    """ark_crypto_primitives::merkle_tree::Path: the sibling of the leaf, the siblings above it from the top down (log_n - 1 of them),
    and the leaf's index"""

    def __init__(self, leaf_sibling_hash, auth_path, leaf_index):
        self.leaf_sibling_hash, self.auth_path, self.leaf_index = leaf_sibling_hash, list(auth_path), leaf_index

    def verify(self, params, root, leaf):
        """leaf: the leaf's elements (an integer for leaf_arity = 1)"""
        cur = CRH.evaluate(params, leaf if isinstance(leaf, (list, tuple)) else [leaf])
        index = self.leaf_index
        for sibling in [self.leaf_sibling_hash] + self.auth_path[::-1]:
            cur = TwoToOneCRH.compress(params, sibling, cur) if index & 1 else TwoToOneCRH.compress(params, cur, sibling)
            index >>= 1
        return cur == int(root) % params.p


class MerkleTree:
    """ark MerkleTree::new(leaf_params, two_to_one_params, leaves) with both parameter sets the same.  nodes: 2n - 1 elements on the
    device, level j (0 = leaf digests) at 2n - 2^(log_n - j + 1), the root last (upstream's heap order is not mirrored)."""

    def __init__(self, params, nodes, log_n):
        self.params, self.nodes, self.log_n, self.n = params, nodes, log_n, 1 << log_n

    @classmethod
    def new(cls, params, leaves_dev, leaf_arity=1, stream=0):
        from .groth16 import _new_buffer
        total = int(np.prod(leaves_dev.shape[:-1]))
        n = total // leaf_arity if leaf_arity >= 1 else 0
        log_n = n.bit_length() - 1
        if n < 2 or n != 1 << log_n or n * leaf_arity != total:       # upstream: assert!(leaf_nodes_size > 1 && is_power_of_two)
            raise ZkError(ZK_ERR_INVALID_ARG, "MerkleTree.new: %d leaf elements at leaf_arity %d are no power of two (> 1) of leaves" % (total, leaf_arity))
        nodes = _new_buffer((2 * n - 1, 4))
        _check(params._lib.zk_poseidon_merkle_tree_device(params.handle, _ptr(leaves_dev), leaf_arity, log_n, _ptr(nodes), ctypes.c_void_p(stream)),
               "zk_poseidon_merkle_tree_device")
        return cls(params, nodes, log_n)

    def root(self):
        from .groth16 import _download
        return from_mont(self.params.p, _download(self.nodes[2 * self.n - 2:2 * self.n - 1]))[0]

    def generate_proofs(self, indices, stream=0):
        from .groth16 import _download, _new_buffer
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        out = _new_buffer((max(len(idx), 1) * self.log_n, 4))
        _check(self.params._lib.zk_merkle_paths_device(self.params.field, _ptr(self.nodes), self.log_n, _ptr(idx), len(idx), _ptr(out), ctypes.c_void_p(stream)),
               "zk_merkle_paths_device")
        sib = from_mont(self.params.p, _download(out))
        return [Path(sib[c * self.log_n], sib[c * self.log_n + 1:(c + 1) * self.log_n][::-1], int(i)) for c, i in enumerate(idx.tolist())]

    def generate_proof(self, index, stream=0):
        return self.generate_proofs([index], stream)[0]

    def free(self):
        self.nodes = None


def elgamal_mask(field, m_dev, dh, out=None, stream=0):
    """EncryptCircuit::encrypt's c2: out[i] = m[i] + dh over a device buffer, dh = CRH of the shared point's affine (x, y) (an
    integer).  The two scalar multiplications on the embedded curve stay with the caller."""
    from .groth16 import _new_buffer
    p = field_modulus(field)
    s = to_mont(p, [dh])
    n = int(np.prod(m_dev.shape[:-1]))
    if out is None:
        out = _new_buffer(tuple(m_dev.shape))
    _call("zk_vec_add_scalar_device", field_id(field), _ptr(out), _ptr(m_dev), n, _ptr(s), ctypes.c_void_p(stream))
    return out


def elgamal_unmask(field, c2_dev, dh, out=None, stream=0):
    """decrypt's mirror: out[i] = c2[i] - dh"""
    return elgamal_mask(field, c2_dev, -int(dh), out, stream)
