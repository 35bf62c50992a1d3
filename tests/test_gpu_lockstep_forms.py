"""Lock-step batches of synthetic shards (zkhip_prove_shards, csrc/batch.h) across the kernel choices that exist only inside a batch:
the proofs of a batch must be byte for byte those of the one-context-per-worker path, and those of the oracle (exact: no tolerance).

Every case: traces from ctx.gen_trace(seed, s) with a shard id of its own per job (gen_trace_logup where the shape has LogUp pairs; for
pitched or unaligned members pitched.embed() of the oracle's trace; for host cases the oracle's trace itself), proven with
set_lockstep(max_batch, lanes) and then with set_lockstep(0) -- the reference --; every proof equal, the first and the last job's equal to
the oracle's on the same trace (module cache), the lock-step counters showing merged launches, pitched inputs unchanged word for word.
With one twin made to read slot 0 instead of slot blockIdx.z (hash_rows_vec_kernel_batch, tried once in a scratch build) exactly the nine
cases whose trees name `vec` fail; test_gpu_lockstep.py::test_small_shards_in_lockstep still passes.

Which kernels a case reaches is established by restated predicates alone: lockstep_forms.py restates coop_max_nodes(), op_merkle_commit,
LaunchBatcher::stage and the cuts of deal_jobs_lockstep, its CASES carry the launches of every case as literals and
test_lockstep_forms_cpu.py holds them to the predicates.  bound = max(512, 16384 / members):

  launcher / choice               inside a batch                                     kernel (batched twin)           cases (ids)
  ------------------------------  -------------------------------------------------  ------------------------------  ---------------------------------
  launch_hash_rows                height <= bound                                    hash_rows16_kernel              every case (trees of <= 512 nodes)
                                  above, W % 4 == 0 (1024 .. 16384 rows)             hash_rows_vec_kernel            n9, n10-stream, n10-level (bound 512),
                                                                                                                     n11-small (4096 rows), n12-*, n13-small
  op_merkle_commit                512 < height <= bound: leaves in the subtree       hash_sub16_kernel, rest 32      n9 (FRI), mixed, host-n9, n12-b3
                                  launch                                             rest 128                        n11-eq (height = bound), n12-b3, n13-small
                                  512 < level <= bound                               compress_sub16_kernel, rest 32  n9, n10-stream, n11-small, n12-small
                                                                                     rest 128                        n12-b3 (bound 5461), n13-small (bound 8192)
  launch_compress_level           count <= bound                                     compress_level16_kernel         512: n10-level, n9-wide .. 8192: n13-small
                                  above (1024 .. 8192 nodes)                         compress_level_kernel           n10-level, n12-b3, n12-small, host-n11
  launch_compress_top             always                                             compress_top16_kernel           512 nodes down to 2
  launch_merkle_p24_rowmajor      hash width 24                                      (width-24 trees)                r0
  launch_ntt_pass                 pair_ok / otherwise, one pass (<= 2^10 rows)       ntt_pass_kernel pair / single   n10-stream, n9-wide / n5 .. n10-level
                                  two passes, one column per lane; 32 + 8 columns                                    n11-eq; n12-b3
  lde_small                       2^11, 2^12 (four cosets, W % 8 == 4), 2^13 rows    lde_small_kernel<1>, <2>, <3>   n11-small, n12-small, n13-small
  launch_quotient                 W % 32 == 0, 2N >= 2048 (at the minimum)           quotient_stream_kernel          n10-stream, mixed, n11-small
                                  otherwise                                          quotient_kernel<1>, <3>, <8>    n5 .., n12-small, n9-wide
  LogUp                           pairs 1: perm trace, its LDE and tree, addend                                      n6-grind, n9, n12-b3
  launch_open                     open_uses_quads / otherwise                        open_partial4 / open_partial    n11-small, n9-wide / the narrow cases
  launch_rowdot                   generic, register forms NK 1, 2, 3                 rowdot(_regs / _stream)_kernel  n5, n9-wide / n9 .. / n11-small / n12-small
  fold                            by 2 launch by launch (no graph); by 16            fri_fold_dev_kernel             every case; r0
  grind_witness                   one window, and a second one for one member        grind_kernel, votes             every case; n6-grind (shards 59, 28)
  dev_h2d / dev_d2h               staged; above half a region: hipMemcpyAsync        copy_bytes_kernel               every case; n9-wide (121 600 B up of
                                                                                                                     64 KiB, 430 400 B down of 384 KiB)
  deal_jobs_lockstep              members ask for different kernels: group by group  (the `mixed` counter)           mixed (ld 32, 36, 33, base off 1)
                                  a batch of one beside a merged one; uneven cuts                                    cuts-2of3 (1 + 2), cuts-4of5 (2 + 3)
  zkhip_prove_shard_host          host traces: hipMemcpyAsync + convert in a batch   convert_kernel                  host-n9 (48 KiB), host-n11 (1 MiB)

Not reachable from a synthetic prove_shards (lockstep_forms.OUT_OF_SCOPE names the predicate and the test that runs each): hash_rows_mvec,
compress_inject_mvec and inject (op_merkle_commit_mixed only), hash_rows_generic and small_eval (check_shape: W % 4 == 0, log_n >= 5).
The file's 17 cases take about 2.5 s on an MI355X, the oracle included (the slowest, n9-wide with its 2 x 64 proofs, 0.3 s).
"""
import pytest

import lockstep_forms as LF
import pitched as PT
from zktls_amd._lib import Params

pytestmark = pytest.mark.gpu

_ORACLE = {}                                     # (case id, job) -> (the oracle's trace, its proof bytes); nobody writes to them


def _oracle_trace(oracle, c, j):
    pairs = c.prm[3]
    if pairs:
        return oracle.gen_trace_logup(LF.SEED, c.shards[j], c.log_n, c.width, pairs)
    return oracle.gen_trace(LF.SEED, c.shards[j], c.log_n, c.width)


def _oracle_proof(oracle, c, j):
    key = (c.id, j)
    if key not in _ORACLE:
        t = _oracle_trace(oracle, c, j)
        t.setflags(write=False)
        _ORACLE[key] = (t, oracle.prove_shard(t, LF.public_values(c, j), oracle.Params(*c.prm)).tobytes())
    return _ORACLE[key]


@pytest.fixture()
def lockstep():
    from zktls_amd.device import set_lockstep
    yield set_lockstep
    set_lockstep(16, 6)                                       # the library's defaults


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in LF.CASES])
def test_lockstep_batches_prove_the_same_bytes(ctx, oracle, lockstep, c):
    from zktls_amd.device import lockstep_stats, prove_shards
    prm = Params(*c.prm)
    n = len(c.shards)
    pvs = [LF.public_values(c, j) for j in range(n)]
    traces, lds, embedded = [], [], []
    for j in range(n):
        ld, off = LF.layout(c, j)
        lds.append(ld)
        if c.host:
            traces.append(_oracle_trace(oracle, c, j))
        elif c.layouts:
            buf, view = PT.embed(ctx, _oracle_trace(oracle, c, j), ld, off)
            embedded.append(buf)
            traces.append(view)
        elif c.prm[3]:
            traces.append(ctx.gen_trace_logup(LF.SEED, c.shards[j], c.log_n, c.width, c.prm[3]))
        else:
            traces.append(ctx.gen_trace(LF.SEED, c.shards[j], c.log_n, c.width))
    kw = dict(device=0, in_flight=4, host=c.host, lds=None if c.host else lds)
    # the batch first: the pooled contexts' workspaces then hold nothing of these shards (the table's shard ids are distinct), so a twin that
    # leaves a member's output unwritten cannot find the reference run's words there
    lockstep(c.max_batch, c.lanes)
    s0 = lockstep_stats()
    got = prove_shards(traces, c.log_n, c.width, pvs, prm, **kw)
    s1 = lockstep_stats()
    lockstep(0)
    ref = prove_shards(traces, c.log_n, c.width, pvs, prm, **kw)
    wrong = [j for j in range(n) if ref[j].size == 0 or got[j].tobytes() != ref[j].tobytes()]
    assert not wrong, "jobs %s of %d differ from the unbatched proofs" % (wrong, n)
    for j in (0, n - 1):
        assert got[j].tobytes() == _oracle_proof(oracle, c, j)[1], "job %d differs from the oracle's proof" % j
    launches, requests, mixed = (s1[k] - s0[k] for k in range(3))
    assert 0 < launches < requests, (launches, requests)      # something merged
    if c.id == "mixed":
        assert mixed > 0                                       # members launched group by group
    for b in embedded:
        PT.assert_unchanged(b)
    for t in (embedded if c.layouts else ([] if c.host else traces)):
        t.free()
