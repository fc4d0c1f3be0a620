// One translation unit per scalar field: hipcc -DZK_FIELD=<PallasFp|PallasFq|Bn254Fr|Bls381Fr>
#include "zk_ntt.inl"
template struct zk::FieldLaunch<zk::ZK_FIELD>;
