"""One rank of the world-2 re-randomization test on ONE GPU (tests/test_rerandomize_gpu.py::
test_world2_rerandomize_gloo_transport; not collected by pytest).  Both ranks share device 0 and exchange through
the test transport (tests/gloo_transport.py), as tests/fanout_gloo_rank.py does.  Every rank installs the same
public key, re-randomizes the broadcast operand under the same derived seed -- no collective: each computes the
same words -- and runs the compat 256-bit product on it with its levels split over the ranks.  Rank 0 then
detaches and repeats both alone: the serialized words of the split run (both ranks) must equal the unsplit
run's.  A NULL seed is refused while the communicator is attached.  Prints one JSON line per rank."""
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
    from fhe_sign import (COMPAT, BigUintFHE, CompactPublicKey, Context, FheError, generate_keys, rerandomization_seed,
                          set_server_key)
    import gloo_transport
    out = {"rank": rank}
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "biguint_vectors.json")))["mul"][0]
    val = lambda limbs: sum(int(x) << (32 * i) for i, x in enumerate(limbs))  # noqa: E731
    a, b = val(golden["a"]), val(golden["b"])
    ck, sk = generate_keys(seed=0x6A12)  # the same client key, hence the same public key, on both ranks
    ck.seed_encryption(0x5EED, 100)
    pk = CompactPublicKey.new(ck, seed=bytes(range(32)))
    ctx = Context(0)
    if rank == 0:
        ctx.set_server_key(sk)
    gloo_transport.attach(ctx, rank, world, min_level=257)
    ctx.broadcast_server_key(0)
    ctx.set_public_key(pk)
    set_server_key(ctx)
    A, B = (BigUintFHE.broadcast(BigUintFHE.new(v, ck) if rank == 0 else None, 0, ctx) for v in (a, b))
    seed = rerandomization_seed(b"tests/rerandomize_gloo_rank", b"request 1")
    try:
        A.re_randomize()
        out["null_refused"] = False
    except FheError as e:
        out["null_refused"] = e.code == -1 and "seed" in str(e)
    _, _, lv0 = ctx.fanout_info()
    R = A.re_randomize(seed)
    out["rerand_sha"] = hashlib.sha256(R.serialize()).hexdigest()
    out["source_sha"] = hashlib.sha256(A.serialize()).hexdigest()
    P = R.mul(B, COMPAT)
    out["compat_ok"] = P.decrypt_limbs(ck) == [int(x) for x in golden["out"]]
    _, _, lv1 = ctx.fanout_info()
    out["split_levels"] = lv1 - lv0
    out["compat_sha"] = hashlib.sha256(P.serialize()).hexdigest()
    dist.barrier()
    ctx.detach_comm()
    if rank == 0:  # the unsplit run on the same input ciphertexts
        R1 = A.re_randomize(seed)
        out["unsplit_rerand_sha"] = hashlib.sha256(R1.serialize()).hexdigest()
        P1 = R1.mul(B, COMPAT)
        out["unsplit_sha"] = hashlib.sha256(P1.serialize()).hexdigest()
        out["unsplit_ok"] = P1.decrypt_limbs(ck) == [int(x) for x in golden["out"]]
    print(json.dumps(out), flush=True)
    dist.barrier()
    set_server_key(None)
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
