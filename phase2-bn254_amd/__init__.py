"""mi355zk: MI355X (gfx950) backend for the BN254 MSM / Fr-NTT hot path of kobigurk/phase2-bn254.

Layout:
  csrc/           hand-written HIP kernels + the C ABI (include/mi355zk.h) -> libmi355zk.so
  lib.py          ctypes loader (fails loudly when the library is missing)
  shard.py        multi-GPU point-range sharding + the all-gather/join exchange step
  generator.py    groth16 generate_parameters (generator.rs:178-510) over fixed-base window tables on the device
  pairing.py      the checking half: pairing products on the device, same_ratio[_batch], prepare_verifying_key, verify_proof[s]
  kzg.py          KZG commitments over an accumulator's tau powers: commit, open, check and their batched forms (csrc/fr_poly.hip: the
                  division by (x - z) and the evaluation on the device)
  grand_product.py  running products and sums of device-resident Fr rows (csrc/fr_scan.hip): prefix_products, prefix_sums, ratio_products,
                  ratio_sums, mul_add; grand_product_polynomials (sonic's GrandProductArgument::new) and permutation_product on top
  keys.py         hash_to_g2, the key pairs and public-key records of both ceremonies (host work on single points)
  verify.py       the ceremony steps and their checks: contribute_mpc_parameters, verify_contribution, verify_mpc_parameters,
                  contribute_response, verify_transform, next_challenge -- one pairing launch per verification
  stream.py       powers-of-tau files streamed through the device in bounded memory: batches, calculate_hash_file, new_constrained,
                  compute_constrained, verify_transform_constrained (file to file, mmap'ed; the in-memory flows of verify.py are the yardstick);
                  prepare_phase2_plan, prepare_phase2_files (a response -> every phase1radix2m{k}, one vector on the device at a time),
                  read_phase1radix2m_file, points_load / points_store (wire records in a mapping <-> a device vector)
  prover.py       the caller of the path: groth16 create_proof (prover.rs:202-343) over the device library; create_proofs: many
                  witnesses of one circuit, each of the eight multiexps one batched call (bellman.multiexp_many)
  ceremony.py     the ceremony-side callers (batch_exp, merge_pairs, QAP evaluation, point FFT, codecs, file containers)
  bellman.py      host-side mirror of the reference's interface for this path:
                  multiexp(), FullDensity, DensityTracker, EvaluationDomain, SynthesisError

The directory name carries a hyphen (it is the reference's name); import it through the
repo-root shim module `phase2_bn254_amd`.
"""
from . import bellman, ceremony, circom, generator, grand_product, keys, kzg, lib, pairing, prover, shard, stream, verify  # noqa: F401
from .bellman import (  # noqa: F401
    DensityTracker,
    EvaluationDomain,
    FixedBaseTable,
    FullDensity,
    MsmTable,
    StridedBases,
    SynthesisError,
    Worker,
    h_poly_host,
    multiexp,
    multiexp_many,
    pin_bases,
    unpin_bases,
)
from .stream import (  # noqa: F401
    batches,
    calculate_hash_file,
    compute_constrained,
    new_constrained,
    points_load,
    points_store,
    prepare_phase2_files,
    prepare_phase2_plan,
    read_phase1radix2m_file,
    verify_transform_constrained,
)
from .verify import (  # noqa: F401
    VerificationError,
    contribute_mpc_parameters,
    contribute_response,
    next_challenge,
    verify_contribution,
    verify_mpc_parameters,
    verify_transform,
)
