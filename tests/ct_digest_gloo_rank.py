"""One rank of the world-2 bound re-randomization test on ONE GPU (tests/test_ct_digest_gpu.py::
test_world2_bound_rerandomize_gloo_transport; not collected by pytest).  Both ranks share device 0 and exchange
through the test transport (tests/gloo_transport.py), as tests/rerandomize_gloo_rank.py does.  Every rank installs
the same public key and calls re_randomize_bound on the broadcast operand: no seed is passed anywhere and there is
no collective -- each rank digests its own replica, derives the same seed and computes the same words.  Rank 0
then detaches and repeats alone: the serialized words of both ranks must equal the single-process run's.  Prints
one JSON line per rank."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from fhe_sign import BigUintFHE, CompactPublicKey, Context, ReRandomizationContext, generate_keys, re_randomize_bound, set_server_key
    import gloo_transport
    out = {"rank": rank}
    value = 0x0123456789ABCDEF_FEDCBA9876543210_0F1E2D3C4B5A6978_8796A5B4C3D2E1F0
    ck, sk = generate_keys(seed=0x6A14)  # the same client key, hence the same public key, on both ranks
    ck.seed_encryption(0x5EED, 100)
    pk = CompactPublicKey.new(ck, seed=bytes(range(32)))
    ctx = Context(0)
    if rank == 0:
        ctx.set_server_key(sk)
    gloo_transport.attach(ctx, rank, world, min_level=257)
    ctx.broadcast_server_key(0)
    ctx.set_public_key(pk)
    set_server_key(ctx)
    A = BigUintFHE.broadcast(BigUintFHE.new(value, ck) if rank == 0 else None, 0, ctx)
    domain, data = b"tests/ct_digest_gloo_rank", b"request 1"
    out["digest"] = A.digest().hex()
    out["seed0"] = ReRandomizationContext(domain).add_bytes(data).add(A).seed(0).hex()
    (R,) = re_randomize_bound(domain, [A], data)  # under the attached communicator, no seed passed
    out["rerand_sha"] = hashlib.sha256(R.serialize()).hexdigest()
    out["source_sha"] = hashlib.sha256(A.serialize()).hexdigest()
    out["value_ok"] = R.to_biguint(ck) == value
    dist.barrier()
    ctx.detach_comm()
    if rank == 0:  # the single-process run on the same input ciphertexts
        out["unsplit_digest"] = A.digest().hex()
        (R1,) = re_randomize_bound(domain, [A], data)
        out["unsplit_rerand_sha"] = hashlib.sha256(R1.serialize()).hexdigest()
    print(json.dumps(out), flush=True)
    dist.barrier()
    set_server_key(None)
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
