"""Multi-GPU plumbing for the first-dimension shard.

The database is partitioned by first-dimension index j across the ranks of one node; every rank sweeps
its shard and produces full-shape partial accumulators (packed words, each 28-bit field already reduced
mod its prime).  One sum-reduce of those words as integers is carry-safe for up to 16 ranks
(16 * 2^28 = 2^32), after which the root reduces each field mod its prime and continues with the
INTT / CRT lift and the folding.  torch.distributed (backend "nccl" = RCCL over xGMI on ROCm, "gloo"
on CPU) carries the single collective; nothing else crosses ranks.
"""
from __future__ import annotations

MAX_RANKS = 16  # carry-safety bound of the packed sum


def shard_range(rank: int, world: int, dim0: int) -> tuple[int, int]:
    """contiguous j-range [j0, j1) of `rank`; dim0 and world are powers of two in every Spiral geometry"""
    if world < 1 or world > MAX_RANKS:
        raise ValueError(f"world size {world} outside [1, {MAX_RANKS}] (packed-sum carry bound)")
    if dim0 % world != 0:
        raise ValueError(f"first dimension {dim0} does not split evenly over {world} ranks")
    per = dim0 // world
    return rank * per, (rank + 1) * per


def _check(name, t, numel=None):
    """what every collective here assumes of its tensors: int64 words (the packed fields are summed as integers), contiguous, of the
    expected size -- a wrong view would not fail inside RCCL, it would silently reduce the wrong bytes (or hang on a size mismatch)"""
    import torch

    if t.dtype != torch.int64 or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise ValueError(f"{name}: expected a contiguous int64 tensor" + (f" of {numel} words" if numel is not None else "") + f", got {t.dtype}, {tuple(t.shape)}, contiguous={t.is_contiguous()}")


def reduce_accumulators(acc, dst: int = 0, group=None):
    """sum the ranks' packed accumulators into rank `dst` (one collective).  `acc` is an int64 tensor
    viewing the words the sweep wrote; the fields never carry into each other (see module docstring)."""
    import torch.distributed as dist

    _check("reduce_accumulators: acc", acc)
    dist.reduce(acc, dst=dst, op=dist.ReduceOp.SUM, group=group)
    return acc


def reduce_scatter_accumulators(chunk, acc, group=None, async_op=False):
    """one collective: every rank receives the element-wise sum of its contiguous chunk of the ranks' accumulator
    buffers (the sweep wrote them grouped by ii mod world, Server.set_fold_ranks).  RCCL has a native reduce-scatter;
    gloo (CPU tests) does not, there the same result is an all-reduce followed by a slice."""
    import torch.distributed as dist

    _check("reduce_scatter_accumulators: acc", acc)
    _check("reduce_scatter_accumulators: chunk", chunk, acc.numel() // dist.get_world_size(group))
    if dist.get_backend(group) == "gloo":
        tmp = acc.clone()
        dist.all_reduce(tmp, op=dist.ReduceOp.SUM, group=group)
        n = chunk.numel()
        chunk.copy_(tmp[dist.get_rank(group) * n:(dist.get_rank(group) + 1) * n])
        return None if async_op else chunk
    work = dist.reduce_scatter_tensor(chunk, acc, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
    return work if async_op else chunk


def acc_position(ii: int, n_ranks: int, num_per: int, n_stages: int = 1) -> int:
    """where the sweep writes ciphertext ii = g + G k of the accumulator buffer (sweep.hip acc_pos): [stage s][rank g][k' < Ls] with
    k = s Ls + k', Ls = num_per / (G K).  One stage = grouped by rank (set_fold_ranks); K stages = every stage a contiguous 1/K of the
    buffer that is reduce-scattered on its own while the next stage sweeps (set_sweep_stages)."""
    g, k = ii % n_ranks, ii // n_ranks
    ls = num_per // (n_ranks * n_stages)
    return ((k // ls) * n_ranks + g) * ls + k % ls


def reduce_scatter_stages(chunk, acc, n_stages: int, group=None, async_op=False, after_stage=None):
    """the pipelined form: stage s's contiguous 1/K of `acc` is reduce-scattered into rows [s L/K, (s+1) L/K) of `chunk`.
    after_stage(s), when given, is called before stage s's collective is issued (the caller launches the sweep of stage s there);
    async_op: returns the Work handles (None entries on gloo, where the collective is synchronous)."""
    if acc.numel() % n_stages or chunk.numel() % n_stages:
        raise ValueError(f"reduce_scatter_stages: {acc.numel()} / {chunk.numel()} words do not split into {n_stages} stages")
    al, cl = acc.numel() // n_stages, chunk.numel() // n_stages
    works = []
    for s in range(n_stages):
        if after_stage is not None:
            after_stage(s)
        works.append(reduce_scatter_accumulators(chunk[s * cl:(s + 1) * cl], acc[s * al:(s + 1) * al], group=group, async_op=async_op))
    return works if async_op else chunk


def all_gather_cts(gathered, ct, group=None):
    """collect the ranks' locally folded ciphertexts in rank order (96 KiB each)"""
    import torch.distributed as dist

    _check("all_gather_cts: ct", ct)
    _check("all_gather_cts: gathered", gathered, ct.numel() * dist.get_world_size(group))
    dist.all_gather_into_tensor(gathered, ct, group=group)
    return gathered


def instances_of_rank(rank: int, world: int, factor: int) -> list[int]:
    """factor-sharded items (an item = `factor` database instances, select_params.py:297-298): rank r holds instances r, r + world, ...; the
    instances are independent -- one query, expanded and converted on every rank, no reduce -- and their responses are gathered"""
    return list(range(rank, factor, world))


def all_gather_instance_responses(gathered, mine, group=None):
    """collect every rank's block of instance responses in rank order: `mine` holds ceil(factor / world) responses of 6 x 2048 words (the ranks
    with one instance fewer leave their last slot unused), `gathered` world such blocks; instance k = slot k // world of rank k % world.  The one
    collective of the factor-sharded path, 96 KiB per instance"""
    import torch.distributed as dist

    _check("all_gather_instance_responses: mine", mine)
    _check("all_gather_instance_responses: gathered", gathered, mine.numel() * dist.get_world_size(group))
    dist.all_gather_into_tensor(gathered, mine, group=group)
    return gathered


def instance_response(gathered, k: int, world: int, slots: int, words: int = 6 * 2048):
    """instance k's response inside the gathered blocks ([world][slots][words])"""
    r, sl = k % world, k // world
    off = (r * slots + sl) * words
    return gathered[off:off + words]


def fold_ranks(world: int, num_per: int) -> int:
    """ranks taking part in the distributed fold: all of them when they divide num_per, else 1 (root folds alone)"""
    return world if world >= 1 and (world & (world - 1)) == 0 and world <= num_per else 1


def all_gather_gsw_bits(gathered, mine, group=None, async_op=False):
    """sharded expansion: collect the ranks' blocks of GSW-bit ciphertexts in rank order (1.8 MiB in all at config 2).
    async_op: returns the Work handle; the collective then runs on the backend's own stream (ordered after what the
    current stream has enqueued so far) and work.wait() makes the current stream wait for it"""
    import torch.distributed as dist

    _check("all_gather_gsw_bits: mine", mine)
    _check("all_gather_gsw_bits: gathered", gathered, mine.numel() * dist.get_world_size(group))
    work = dist.all_gather_into_tensor(gathered, mine, group=group, async_op=async_op)
    return work if async_op else gathered


def expand_shard_ok(shape, params, world: int) -> bool:
    """can the expansion be sharded over `world` ranks: query compression with the reordered layout, power-of-two ranks"""
    return world >= 1 and (world & (world - 1)) == 0 and not params.direct_upload and shape.stopround > 0 and world <= shape.dim0


# ---- batches of a sharded answer (include/spiral_gpu.h run_pre_sweep_batch ... fold_root_batch) -------------------------------------------------
CT_WORDS = 6 * 2048  # one n1 x n2 ciphertext: 96 KiB
MAX_BATCH = 8        # clients per batch step (the query lanes of one launch)


def _batch_n(n: int) -> int:
    if not 1 <= n <= MAX_BATCH:
        raise ValueError(f"a batch holds 1 .. {MAX_BATCH} clients, got {n}")
    return n


def batch_acc_words(shape, n: int) -> int:
    """words of one rank's rank-major accumulator buffer [rank][lane][num_per / G][CT] (the reduce-scatter's input)"""
    return _batch_n(n) * shape.num_per * CT_WORDS


def batch_chunk_words(shape, n: int, G: int) -> int:
    """words of rank g's reduce-scattered chunk [lane][num_per / G][CT] (fold_local_batch's input)"""
    if G < 1 or shape.num_per % G:
        raise ValueError(f"{G} fold ranks do not divide num_per = {shape.num_per}")
    return _batch_n(n) * (shape.num_per // G) * CT_WORDS


def batch_ct_words(n: int) -> int:
    """words of fold_local_batch's output [lane][CT] (the all-gather's input; also the responses output)"""
    return _batch_n(n) * CT_WORDS


def batch_gathered_ct_words(n: int, G: int) -> int:
    """words of the all-gathered [rank][lane][CT] (fold_root_batch's input)"""
    return G * batch_ct_words(n)


def batch_bits_words(gsw_bits_words: int, n: int) -> int:
    """words of one rank's [lane][gsw_bits_words] block of a sharded expansion (the all-gather's input; x world = its output)"""
    return _batch_n(n) * gsw_bits_words


def batch_acc_position(ii: int, lane: int, n: int, G: int, num_per: int) -> int:
    """where the batch sweep writes lane b's ciphertext ii = g + G k (in ciphertexts): (g n + b) L + k, L = num_per / G -- reduce-scattered, rank g
    receives [lane][k]"""
    L = num_per // G
    g, k = ii % G, ii // G
    return (g * n + lane) * L + k


def batch_collective_bytes(shape, n: int, G: int, gsw_bits_words: int = 0) -> dict:
    """bytes each collective of one batch step moves per rank, from the shapes alone (nothing timed): the accumulator reduce-scatter (its input; with
    G = 1 the reduce to the root), the all-gather of the folded ciphertexts (its output) and, with a sharded expansion, the all-gather of the GSW bits
    (its output)"""
    out = {"reduce_scatter_in_bytes" if G > 1 else "reduce_in_bytes": batch_acc_words(shape, n) * 8}
    if G > 1:
        out["all_gather_cts_out_bytes"] = batch_gathered_ct_words(n, G) * 8
    if gsw_bits_words:
        out["all_gather_bits_out_bytes"] = G * batch_bits_words(gsw_bits_words, n) * 8
    return out


def batch_buffers(servers, world: int, fold_ranks: int, sharded_expansion: bool, device=None) -> dict:
    """the device buffers of one rank's batch steps (int64 tensors, zeroed), sized for len(servers) clients.  Keep them across batches: the calls'
    hipGraphs are keyed by these pointers"""
    import torch

    n, s = _batch_n(len(servers)), servers[0].shape
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    z = lambda words: torch.zeros(words, dtype=torch.int64, device=dev)
    b = {"acc": z(batch_acc_words(s, n)), "cts": z(batch_ct_words(n)), "responses": z(batch_ct_words(n))}
    if fold_ranks > 1:
        b["chunk"] = z(batch_chunk_words(s, n, fold_ranks))
        b["gathered_cts"] = z(batch_gathered_ct_words(n, fold_ranks))
    if sharded_expansion:
        w = servers[0].gsw_bits_words()
        b["bits"] = z(batch_bits_words(w, n))
        b["gathered_bits"] = z(world * batch_bits_words(w, n))
    return b


def reduce_scatter_batch(chunk, acc, group=None, async_op=False):
    """the batch's one accumulator reduce-scatter: acc is rank-major [rank][lane][k], so rank g's contiguous slice is its [lane][k] chunk"""
    return reduce_scatter_accumulators(chunk, acc, group=group, async_op=async_op)


def all_gather_batch_cts(gathered, cts, group=None):
    """the batch's one all-gather of the locally folded ciphertexts: [lane][CT] per rank -> [rank][lane][CT]"""
    return all_gather_cts(gathered, cts, group=group)


def all_gather_batch_bits(gathered, bits, group=None, async_op=False):
    """the batch's one all-gather of the GSW bits of a sharded expansion: [lane][words] per rank -> [rank][lane][words]"""
    return all_gather_gsw_bits(gathered, bits, group=group, async_op=async_op)


def answer_batch_sharded(servers, group=None, bufs=None, *, fold_ranks=None, sharded_expansion=False, root=0, wire_ptr: int = 0):
    """One rank's whole answer of a batch of up to eight clients on a j-sharded database, in order: pre + sweep (with a sharded expansion: expand + pack,
    all-gather, unpack + convert + sweep), ONE reduce-scatter of the rank-major accumulators, fold_local_batch, ONE all-gather, fold_root_batch on
    `root`.  fold_ranks = 1 (servers set up with set_fold_ranks(1)): a reduce(SUM) to the root, which folds alone.  servers: this rank's owner (created
    on its j-shard, set_fold_ranks(G), with sharded_expansion also set_expand_shard(rank, world)) and its lanes, each with its client's public
    parameters and query set.  bufs: batch_buffers(...) (allocated here when None; keep them across batches).  Returns bufs; on the root every lane's
    BUF_FINAL / BUF_RESPONSE hold its answer and bufs["responses"] the [lane][CT] responses (wire_ptr: optional device [lane] wire forms)."""
    import torch
    import torch.distributed as dist

    from . import server as SV

    n = _batch_n(len(servers))
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    G = world if fold_ranks is None else fold_ranks
    if G not in (1, world):
        raise ValueError(f"fold ranks must be 1 or the world size {world}, got {G}")
    if world > MAX_RANKS:
        raise ValueError(f"world size {world} above the packed-sum carry bound {MAX_RANKS}")
    if bufs is None:
        bufs = batch_buffers(servers, world, G, sharded_expansion)
    s = servers[0].shape
    _check("answer_batch_sharded: acc", bufs["acc"], batch_acc_words(s, n))
    _check("answer_batch_sharded: cts", bufs["cts"], batch_ct_words(n))
    _check("answer_batch_sharded: responses", bufs["responses"], batch_ct_words(n))

    def settle():  # the servers' stream -> the collective (on torch's stream) -> the servers' stream
        servers[0].sync()

    def landed():
        torch.cuda.current_stream(bufs["acc"].device).synchronize()

    if sharded_expansion:
        SV.run_expand_pack_batch(servers, bufs["bits"].data_ptr())
        settle()
        all_gather_batch_bits(bufs["gathered_bits"], bufs["bits"], group=group)
        landed()
        SV.run_unpack_convert_sweep_batch(servers, bufs["gathered_bits"].data_ptr(), bufs["acc"].data_ptr())
    else:
        SV.run_pre_sweep_batch(servers, bufs["acc"].data_ptr())
    settle()
    if G == 1:
        reduce_accumulators(bufs["acc"], dst=root, group=group)
        landed()
        if rank == root:
            SV.fold_local_batch(servers, bufs["acc"].data_ptr(), bufs["cts"].data_ptr())
            SV.fold_root_batch(servers, bufs["cts"].data_ptr(), bufs["responses"].data_ptr(), wire_ptr)
            settle()
        return bufs
    reduce_scatter_batch(bufs["chunk"], bufs["acc"], group=group)
    landed()
    SV.fold_local_batch(servers, bufs["chunk"].data_ptr(), bufs["cts"].data_ptr())
    settle()
    all_gather_batch_cts(bufs["gathered_cts"], bufs["cts"], group=group)
    landed()
    if rank == root:
        SV.fold_root_batch(servers, bufs["gathered_cts"].data_ptr(), bufs["responses"].data_ptr(), wire_ptr)
        settle()
    return bufs


# ---- batches on a column-sharded database (include/spiral_gpu.h create_column_shard, run_column_batch) -----------------------------------------
def column_batch_collective_bytes(shape, n: int, G: int) -> dict:
    """bytes the ONE collective of a column-sharded batch step moves per rank, from the shapes alone (nothing timed): the all-gather of the locally
    folded ciphertexts (its output, [rank][lane][CT]).  Nothing is reduced: every rank's sweep yields finished sums for its own columns"""
    if G < 1 or (G & (G - 1)) or shape.num_per % G:
        raise ValueError(f"{G} column shards do not divide num_per = {shape.num_per}")
    return {"all_gather_cts_out_bytes": batch_gathered_ct_words(n, G) * 8}


def column_batch_buffers(servers, world: int, device=None) -> dict:
    """the device buffers of one rank's column-sharded batch steps (int64 tensors, zeroed), sized for len(servers) clients: "cts" (run_column_batch's
    output, the all-gather's input), "gathered_cts" and "responses".  No accumulator buffer and no chunk: the sweep writes the lanes' own
    accumulators.  Keep them across batches: the calls' hipGraphs are keyed by these pointers"""
    import torch

    n = _batch_n(len(servers))
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    z = lambda words: torch.zeros(words, dtype=torch.int64, device=dev)
    return {"cts": z(batch_ct_words(n)), "gathered_cts": z(batch_gathered_ct_words(n, world)), "responses": z(batch_ct_words(n))}


def answer_batch_column_sharded(servers, group=None, bufs=None, *, root=0, wire_ptr: int = 0):
    """One rank's whole answer of a batch of up to eight clients on a column-sharded database, in order: run_column_batch (expansion, conversion, the
    sweep of this rank's columns and the local fold rounds), ONE all-gather of the folded ciphertexts, fold_root_batch on `root`.  servers: this rank's
    column shard owner (Server(params, col_rank=rank, col_ranks=world)) and its lanes, each with its client's public parameters and query set.  bufs:
    column_batch_buffers(...) (allocated here when None; keep them across batches).  Returns bufs; on the root every lane's BUF_FINAL / BUF_RESPONSE
    hold its answer and bufs["responses"] the [lane][CT] responses (wire_ptr: optional device [lane] wire forms).  The servers' stream is settled
    before the collective (on torch's stream) and the collective before the root's fold, as in answer_batch_sharded"""
    import torch
    import torch.distributed as dist

    from . import server as SV

    n = _batch_n(len(servers))
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    if (servers[0].col_rank, servers[0].col_ranks) != (rank, world):
        raise ValueError(f"rank {rank} of {world} needs column shard {rank} of {world}, the servers are {servers[0].col_rank} of {servers[0].col_ranks}")
    if bufs is None:
        bufs = column_batch_buffers(servers, world)
    _check("answer_batch_column_sharded: cts", bufs["cts"], batch_ct_words(n))
    _check("answer_batch_column_sharded: gathered_cts", bufs["gathered_cts"], batch_gathered_ct_words(n, world))
    _check("answer_batch_column_sharded: responses", bufs["responses"], batch_ct_words(n))

    def settle():  # the servers' stream -> the collective (on torch's stream) -> the servers' stream
        servers[0].sync()

    def landed():
        torch.cuda.current_stream(bufs["cts"].device).synchronize()

    SV.run_column_batch(servers, bufs["cts"].data_ptr())
    settle()
    all_gather_batch_cts(bufs["gathered_cts"], bufs["cts"], group=group)
    landed()
    if rank == root:
        SV.fold_root_batch(servers, bufs["gathered_cts"].data_ptr(), bufs["responses"].data_ptr(), wire_ptr)
        settle()
    return bufs


# ---- SpiralPack batches on trial-sharded servers (include/spiral_gpu.h fold_trials_batch, pack_gathered_batch) ----------------------------------
PACK_CT_WORDS = 2 * 2048  # one folded SpiralPack ciphertext (2 x 1 polynomials, raw words): 32 KiB


def pack_trial_cuts(world: int, trials: int) -> list[int]:
    """the ranks' trial ranges: rank r holds [cuts[r], cuts[r + 1]), consecutive, covering [0, trials), sizes differing by at most one (trials need not
    divide by world; every rank holds at least one trial)"""
    if world < 1 or world > trials:
        raise ValueError(f"{world} ranks for {trials} trials: every rank holds at least one")
    return [r * trials // world for r in range(world + 1)]


def _pack_cuts(cuts) -> list[int]:
    cuts = [int(c) for c in cuts]
    if len(cuts) < 2 or cuts[0] != 0 or any(b <= a for a, b in zip(cuts[:-1], cuts[1:])):
        raise ValueError(f"trial cuts {cuts}: they start at 0 and increase strictly")
    return cuts


def pack_batch_block_cts(n: int, cuts) -> int:
    """ciphertexts of one rank's block of the all-gather, [lane][k]: n lanes x the LONGEST range, the same on every rank (an all-gather takes equal
    blocks; a shorter range leaves the tail of its block as padding, which nothing reads)"""
    cuts = _pack_cuts(cuts)
    return _batch_n(n) * max(b - a for a, b in zip(cuts[:-1], cuts[1:]))


def pack_batch_position(rank: int, lane: int, k: int, n: int, cuts, block_cts: int) -> int:
    """where lane b's folded ciphertext of trial cuts[rank] + k lies in the gathered buffer (in ciphertexts): rank-major blocks at a stride of
    block_cts, inside a block [lane][k < the rank's range]"""
    cuts = _pack_cuts(cuts)
    if not 0 <= rank < len(cuts) - 1:
        raise ValueError(f"rank {rank} outside the {len(cuts) - 1} ranks of the cuts")
    length = cuts[rank + 1] - cuts[rank]
    if not 0 <= lane < _batch_n(n) or not 0 <= k < length:
        raise ValueError(f"lane {lane} of {n}, trial {k} of rank {rank}'s {length}")
    if block_cts < n * length:
        raise ValueError(f"blocks of {block_cts} ciphertexts do not hold {n} lanes of {length} trials")
    return rank * block_cts + lane * length + k


def pack_batch_buffers(servers, cuts, device=None) -> dict:
    """the two device buffers of one rank's trial-sharded batches (int64 tensors, zeroed), sized for len(servers) clients: "mine", this rank's block
    (fold_trials_batch's output, the all-gather's input), and "gathered", the ranks' blocks.  Keep them across batches"""
    import torch

    cuts = _pack_cuts(cuts)
    block = pack_batch_block_cts(len(servers), cuts)
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return {"mine": torch.zeros(block * PACK_CT_WORDS, dtype=torch.int64, device=dev),
            "gathered": torch.zeros((len(cuts) - 1) * block * PACK_CT_WORDS, dtype=torch.int64, device=dev), "block_cts": block}


def all_gather_pack_batch(gathered, mine, group=None):
    """the batch's one collective: every rank's block [lane][k] (padded to the common size) -> [rank][lane][k]; n x out_n^2 x 32 KiB of payload"""
    import torch.distributed as dist

    _check("all_gather_pack_batch: mine", mine)
    _check("all_gather_pack_batch: gathered", gathered, mine.numel() * dist.get_world_size(group))
    dist.all_gather_into_tensor(gathered, mine, group=group)
    return gathered


def answer_pack_batch_sharded(servers, queries, group=None, bufs=None, *, form="ntt", root=0, wire=False):
    """One rank's whole answer of a batch of up to eight SpiralPack clients on trial-sharded servers, in order: fold_trials_batch over this rank's trials,
    ONE all-gather of the ranks' blocks, pack_gathered_batch on `root`.  servers: this rank's owner -- created for the trials
    pack_trial_cuts(world, out_n^2)[rank : rank + 2] -- and / or its shard lanes (create_shard_lane), lane b with client b's public parameters on every
    rank; queries: the clients' queries, the same on every rank.  bufs: pack_batch_buffers(...) (allocated here when None; keep them across
    batches).  Returns (bufs, out): out is pack_gathered_batch's result on the root, None elsewhere.  The servers' stream is settled before the
    collective (which runs on torch's current stream) and the collective before the pack, as in answer_batch_sharded."""
    import torch
    import torch.distributed as dist

    from .pack import fold_trials_batch, pack_gathered_batch  # (spiral_amd.pack is also the name of a function: take the module's own)

    n = _batch_n(len(servers))
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    s0 = servers[0]
    cuts = pack_trial_cuts(world, s0.shape.trials)
    if (s0.trial0, s0.trial1) != (cuts[rank], cuts[rank + 1]):
        raise ValueError(f"rank {rank} of {world} holds trials [{cuts[rank]}, {cuts[rank + 1]}), the servers [{s0.trial0}, {s0.trial1})")
    if bufs is None:
        bufs = pack_batch_buffers(servers, cuts)
    block = pack_batch_block_cts(n, cuts)
    _check("answer_pack_batch_sharded: mine", bufs["mine"], block * PACK_CT_WORDS)
    _check("answer_pack_batch_sharded: gathered", bufs["gathered"], world * block * PACK_CT_WORDS)
    dev = bufs["mine"].device
    fold_trials_batch(servers, queries, bufs["mine"].data_ptr(), form=form)
    torch.cuda.synchronize(dev)  # the servers' stream -> the collective (on torch's stream)
    all_gather_pack_batch(bufs["gathered"], bufs["mine"], group=group)
    torch.cuda.current_stream(dev).synchronize()  # the collective -> the servers' stream
    out = None
    if rank == root:
        out = pack_gathered_batch(servers, bufs["gathered"].data_ptr(), cuts, block, wire=wire)
    return bufs, out
