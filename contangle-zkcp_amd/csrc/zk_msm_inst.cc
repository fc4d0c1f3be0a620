// One translation unit per curve: hipcc -DZK_CURVE=<Pallas|Vesta|Bn254G1|Bls381G1|Bn254G2|Bls381G2>
#include "zk_msm.inl"
template struct zk::CurveLaunch<zk::ZK_CURVE>;
