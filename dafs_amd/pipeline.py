"""Host-side driver of the whole DAFS run on top of the C ABI -- the Python mirror of
DAFS::run (reference src/dafs.cpp:1781-1889) used by tests and bench.py.  Everything numeric is
done by libdafs_hip.so on the GPU; this file only holds the schedule, the alignment bookkeeping
(project_alignment) and the FASTA-style output.  The C++ `dafs` executable (dafs_amd/csrc/host/cli_main.cpp)
is the same logic for the drop-in command line; the guide tree, the Stockholm block, the tables and the memory estimates
of both are the library's host code (dafs_amd/csrc/host_tree.cpp, host_text.cpp)."""
import inspect
import os
import sys

import numpy as np

from . import capi, stockholm

NONE = 0xFFFFFFFF


def tree_string(score, left, right, names, i=None):
    """print_tree, src/dafs.cpp:495-511 (operator<<(float) == %g)"""
    if i is None:
        i = len(score) - 1
    if left[i] < 0:
        return names[i]
    return "[ %g %s %s ]" % (float(score[i]), tree_string(score, left, right, names, left[i]),
                            tree_string(score, left, right, names, right[i]))


def project_alignment(a1, a2, z):
    """src/dafs.cpp:766-825.  a = (seq_idx[n], mask[n, L])"""
    s1, m1 = a1
    s2, m2 = a2
    L1, L2 = m1.shape[1], m2.shape[1]
    cols1, cols2 = [], []  # per output column: source column in aln1 / aln2 or -1
    k = 0
    for i in range(L1):
        if z[i] != NONE:
            while k < z[i]:
                cols1.append(-1); cols2.append(k); k += 1
            cols1.append(i); cols2.append(k); k += 1
        else:
            cols1.append(i); cols2.append(-1)
    while k < L2:
        cols1.append(-1); cols2.append(k); k += 1
    c1 = np.array(cols1); c2 = np.array(cols2)
    o1 = np.where(c1[None, :] >= 0, m1[:, np.maximum(c1, 0)], 0).astype(np.uint8)
    o2 = np.where(c2[None, :] >= 0, m2[:, np.maximum(c2, 0)], 0).astype(np.uint8)
    return np.concatenate([s1, s2]), np.concatenate([o1, o2], axis=0)


class Result:
    pass


DECODERS = ("Nussinov", "Levels")


class LevelThresholds(tuple):
    """th_s1 of a run with decoder="Levels" once its options are checked (decoder_option): one threshold per level"""


def decoder_option(decoder, th_s, th_s1, bp_update1=False, seed_ss=None, who="pipeline.run"):
    """The final decode of a driver from its options decoder, th_s, th_s1, checked before any work.
    Returns what the driver then carries as th_s1: for "Nussinov" th_s1 itself, or its first entry when it is a sequence;
    for "Levels" a LevelThresholds of every entry (of th_s1, else th_s, when a scalar).  Refused: an unknown decoder, more
    than capi.MAX_LEVELS thresholds, a threshold of a higher level that is not positive, and "Levels" with bp_update1 or with
    a seed structure.  th_s1 a capi.AutoThresholds: the thresholds are chosen by pseudo-expected accuracy
    and the object is carried as it is; refused with bp_update1 (what the second decode would mean is undecided), with a seed
    structure (nothing is decoded), with more than one level under "Nussinov", and as th_s, the threshold inside the loop."""
    if isinstance(th_s1, LevelThresholds):
        return th_s1
    if decoder not in DECODERS:
        raise ValueError("%s: unknown decoder %r (one of %s)" % (who, decoder, ", ".join(DECODERS)))
    if isinstance(th_s, capi.AutoThresholds):
        raise ValueError("%s: th_s, the threshold inside the dual-decomposition loop, cannot be chosen automatically; "
                         "th_s1 can" % who)
    if isinstance(th_s1, capi.AutoThresholds):
        if bp_update1:
            raise ValueError("%s: automatic thresholds cannot be combined with bp_update1" % who)
        if seed_ss is not None:
            raise ValueError("%s: with seed_ss nothing is decoded: automatic thresholds cannot be combined with it" % who)
        if decoder == "Nussinov" and th_s1.levels != 1:
            raise ValueError("%s: decoder \"Nussinov\" decodes one level; automatic thresholds of %d levels need decoder "
                             "\"Levels\"" % (who, th_s1.levels))
        return th_s1
    ths = None
    if th_s1 is not None and np.ndim(th_s1) != 0:
        ths = [float(x) for x in th_s1]
        if not 1 <= len(ths) <= capi.MAX_LEVELS:
            raise ValueError("%s: th_s1 holds %d thresholds; one to %d levels are decoded" % (who, len(ths), capi.MAX_LEVELS))
    if decoder == "Nussinov":
        return th_s1 if ths is None else ths[0]
    if bp_update1:
        raise ValueError("%s: decoder \"Levels\" with bp_update1 is not built: the reference folds again per level, under each "
                         "level's constraint" % who)
    if seed_ss is not None:
        raise ValueError("%s: with seed_ss nothing is decoded: decoder \"Levels\" cannot be combined with it" % who)
    if ths is None:
        ths = [float(th_s if th_s1 is None else th_s1)]
    if any(not x > 0.0 for x in ths[1:]):
        raise ValueError("%s: the thresholds of the levels above the first must be positive" % who)
    return LevelThresholds(ths)


def _decode(ctx, alns, th1):
    """The first decode of many final alignments in one call: per alignment (ss, level, scores, auto); level and scores are
    None under the plain decoder (th1 a number), the level array and the per-level scores under th1 a LevelThresholds or a
    capi.AutoThresholds; auto is the capi.AutoChoice of the latter, else None"""
    if isinstance(th1, capi.AutoThresholds):
        return [(ss, level, scores, auto) for scores, ss, level, auto in ctx.consensus_structures(alns, th1)]
    if isinstance(th1, LevelThresholds):
        return [(ss, level, scores, None) for scores, ss, level in ctx.consensus_structures(alns, th1)]
    return [(ss, None, None, None) for _, ss in ctx.consensus_structures(alns, th1)]


def _by_level(th):
    """the decode at th returns levels"""
    return isinstance(th, (LevelThresholds, capi.AutoThresholds))


def run(names, seqs, ctx=None, bp=None, w=4.0, eta0=0.5, t_max=600, w_pct_a=0.25, w_pct_s=0.25, th_a=0.01,
        th_s=0.2, th_s1=None, align_model=capi.ALIGN_PROBCONS, force_iters=0, timers=None, level_sync=False, slice_iters=None,
        mp=None, skip_uncoupled_folds=True, shard=None, round_us=None, w_pct_f=0.0, bp_update=False, bp_update1=False,
        reliability=False, covariation=False, row_structures=False, identity=False, compare=None, phylogeny=False,
        phylogeny_bootstrap=0, phylogeny_seed=12345, decoder="Nussinov", phylogeny_transfer=False):
    """The whole run.  bp: per-sequence (rowptr, col, val) base-pairing rows (--fold-aux); None
    computes them with the device fold model.  mp: supplied matching probabilities (--align-aux), see Context.set_mp.
    shard: (torch.distributed module, torch device) of an initialised process group -- phase 1 (folds, pair posteriors,
    matching consistency transform) is then split over the ranks and gathered (dist.phase1_sharded); every rank
    finishes the run and holds the same result.  reliability: the result also gets .reliability and .stockholm (see
    _phase2_forest).  covariation: True or a dict with shuffles (100), seed (1), e_max (0.05), null ("shuffle"): the result also gets
    .covariation (see _final).  row_structures: the result also gets .row_ss and .row_ss_str, the structure of every printed
    row on its own (see _phase2_forest).  identity: the result also gets .identity (see alignment_identity) and its
    Stockholm block the `#=GS <name> WT` lines.  compare: (ref_names, ref_rows[, ref_ss]), a reference alignment of the same
    sequences as stockholm.read_seed_structure returns it: the result also gets .compare (see compare).  phylogeny: "jc" or
    "p": the result also gets .phylogeny (see alignment_phylogeny), the neighbour-joining tree of the printed rows;
    phylogeny_bootstrap: that many bootstrap replicates drawn from phylogeny_seed: .phylogeny also gets
    .support, .replicates, .seed and .support_table, and .newick carries the support in percent as the labels of the joins.
    phylogeny_transfer (with replicates): .phylogeny also gets .transfer and .depth, .newick carries the
    transfer bootstrap expectation in percent instead and .support_table is the transfer table.
    decoder: "Nussinov", or "Levels" (DESIGN.md section 25): the common structure is decoded level by level at the
    thresholds th_s1 (a sequence, one per level; a scalar or None: one level) and may hold pseudoknots.  .ss is then the
    union of the levels, .ss_level the level of the pair at each of its columns (0xFF at unpaired ones), .ss_scores the
    per-level scores, and .ss_str, the Stockholm SS_cons and the per-row structures print "()", "[]", "{}", "<>" for levels
    0..3.  With "Nussinov" only the first entry of a sequence th_s1 is used.  th_s1 a capi.AutoThresholds (DESIGN.md section
    27): every level's threshold is chosen from its candidates by pseudo-expected accuracy, up to its .levels levels under
    "Levels" and one under "Nussinov"; the result gets .ss_level and .ss_scores as under "Levels" and .ss_auto, the
    capi.AutoChoice (chosen, thresholds, sum_p, tp, npairs, the candidates' table, f); with row_structures every row chooses
    its own thresholds (.row_ss_auto)."""
    import time
    th_s1 = decoder_option(decoder, th_s, th_s1, bp_update1, None, "pipeline.run")
    phylogeny = phylogeny_option(phylogeny, phylogeny_bootstrap, phylogeny_seed, phylogeny_transfer)
    # combinations this driver does not implement are refused, not ignored (the command line, cli_main.cpp, has no level
    # batches: its --bp-update runs in the resident-node rounds and in the refinement's solve_node)
    if level_sync and bp_update:
        raise ValueError("pipeline.run: bp_update needs the resident-node schedule (level_sync=False)")
    if shard is not None and (bp is not None or mp is not None or w_pct_f != 0.0):
        raise ValueError("pipeline.run: a sharded phase 1 computes its posteriors itself: bp / mp (--fold-aux / --align-aux) and "
                         "w_pct_f (-f) are single-process options")
    own = ctx is None
    if own:
        ctx = capi.Context(0)
    t = [time.perf_counter()]
    if shard is not None:
        from . import dist as ddist
        ddist.phase1_sharded(ctx, seqs, shard[0], shard[1], align_model, th_a, w_pct_a, w_pct_s)
        t += [time.perf_counter()] * 2
        sim = ctx.sim()
    else:
        sim = _phase1_local(ctx, seqs, bp, mp, align_model, th_a, w_pct_a, w_pct_s, t, w_pct_f)
    score, left, right = capi.build_tree(sim)  # same code as the command line
    t.append(time.perf_counter())
    fam = dict(names=names, seqs=seqs, first=0, sim=sim, tree=(score, left, right))
    return _phase2_forest(ctx, own, [fam], t, w, eta0, t_max, th_a, th_s, th_s1, force_iters, level_sync, slice_iters,
                          skip_uncoupled_folds, round_us, bp_update, bp_update1, reliability, covariation, row_structures, identity, compare,
                          phylogeny)[0]


def _phase1_local(ctx, seqs, bp, mp, align_model, th_a, w_pct_a, w_pct_s, t, w_pct_f=0.0, first=None, constraints=None):
    """Phase 1 on the context: folds, pair posteriors, consistency transforms.  first: family partition (run_batch); the
    result is then the list of the families' similarity blocks instead of one matrix.  constraints: per sequence a folding
    constraint or None (Context.fold_begin)."""
    import time
    ctx.set_sequences(seqs)
    if first is not None and len(first) > 2:
        ctx.set_families(first)
    # The folding (one workgroup per sequence) leaves most of the device idle, and nothing before the base-pair
    # transform needs its result: it is started on its own stream, and the all-pairs alignment posteriors and the
    # matching-probability transform run beside it.
    folding = False
    try:
        if bp is not None:
            ctx.set_bp(bp)
        else:
            ctx.fold_begin(0.01, constraints=constraints)
            folding = True
        t.append(time.perf_counter())
        if mp is not None:
            ctx.set_mp(*mp)  # (nnz, rowptr, col, val) of every pair, --align-aux
        else:
            ctx.align_posteriors(align_model, th_a, fetch=False)
        t.append(time.perf_counter())
        if w_pct_f != 0.0:  # relax_fourway_consistency (dafs.cpp:1808): needs the base-pairing rows, replaces mp_ before sim_
            if folding:
                folding = False
                ctx.fold_end()
            ctx.fourway_consistency(w_pct_f)
        sim = ctx.sim() if first is None or len(first) <= 2 else ctx.sim_blocks()
        ctx.consistency_match(w_pct_a)
        if folding:
            folding = False
            ctx.fold_end()
        ctx.consistency_bp(w_pct_s)
    except Exception:
        if folding:  # the folding kernels still own their workspaces: wait for them, so that the context can be used again
            try:
                ctx.fold_end()
            except Exception:
                pass
        raise
    return [sim] if first is not None and len(first) <= 2 else sim


def forest_ready(trees, pending, done):
    """The nodes of `pending` ((family, node) in scheduling order) whose two children are in `done`, in that order.
    trees[f] = (left, right) of family f's guide tree (leaves -1)."""
    return [(f, i) for f, i in pending if (f, trees[f][0][i]) in done and (f, trees[f][1][i]) in done]


def _solve_nodes(ctx, prm, take_ready, finish, level_sync=False, slice_iters=None, round_us=None):
    """The node schedule of _phase2_forest and add.  take_ready() returns [(key, node)] for the nodes that have just become
    ready (node: a Context.solve_nodes tuple); it is called once per level or round, after the last one's finished nodes
    have gone to finish(key, out, dims) (dims: (len1, len2), None in level mode).  level_sync: one blocking solve_nodes call
    per batch.  Otherwise the nodes stay resident and a round is one Context.nodes_round call, old handles in key order,
    that ends after round_us microseconds or slice_iters iterations of every node (results do not depend on the cut).
    Returns (levels, per round (seconds from take_ready() to the end of the call, [(key, len1, len2)]), nodes_memory(),
    nodes_demotions()); in level mode the last three are [], None, None."""
    import time
    if level_sync:
        levels = 0
        while True:
            ready = take_ready()
            if not ready:
                return levels, [], None, None
            for (k, _), o in zip(ready, ctx.solve_nodes([node for _, node in ready], prm)):
                finish(k, o, None)
            levels += 1
    if slice_iters is None and round_us is None:
        round_us = int(os.environ.get("DAFS_ROUND_US", "2500"))
    open_nodes = {}  # key -> (handle, len1, len2)
    rounds = []
    while True:
        t_round = time.perf_counter()
        ready = take_ready()
        if not ready and not open_nodes:
            break
        ids, new = sorted(open_nodes), [k for k, _ in ready]
        hs, dims, fin_old, fin_new = ctx.nodes_round([node for _, node in ready], [open_nodes[k][0] for k in ids], prm, slice_iters or 0,
                                                     round_us or 0)
        for k, h, d in zip(new, hs, dims):
            open_nodes[k] = (h, d[0], d[1])
        rounds.append((time.perf_counter() - t_round, [(k, open_nodes[k][1], open_nodes[k][2]) for k in ids + new]))
        for k, fin in list(zip(ids, fin_old)) + list(zip(new, fin_new)):
            if fin:
                h, l1, l2 = open_nodes.pop(k)
                finish(k, ctx.nodes_result(h, l1, l2), (l1, l2))
    memory = ctx.nodes_memory()  # (reserved, in use, peak) bytes of the resident nodes
    demotions = ctx.nodes_demotions()  # split nodes that lost their folders (0 on an undisturbed device)
    ctx.nodes_close()
    return len(rounds), rounds, memory, demotions


def _phase2_forest(ctx, own, fams, t, w, eta0, t_max, th_a, th_s, th_s1, force_iters, level_sync, slice_iters,
                   skip_uncoupled_folds, round_us=None, bp_update=False, bp_update1=False, reliability=False, covariation=False,
                   row_structures=False, identity=False, compare=None, phylogeny=False):
    """The progressive phase and the output of every family of the context at once.  fams: per family a dict with names,
    seqs, first (index of its first sequence in the context), sim and tree = (score, left, right).  The guide trees form one
    forest: a node is ready when both of its children are done, whatever its family, and the ready nodes of all families
    share each launch.  Returns one Result per family.
    reliability: each Result also gets .reliability, the annotation of its final alignment and structure from the stores
    the progressive phase read (one Context.alignment_reliabilities call over all families): a dict with residue (per printed row, its residues'
    values), col, pair, pair_rows and expected_accuracy; and .stockholm, that alignment as a Stockholm block with PP lines
    (dafs_amd/stockholm.py: the block `dafs --stockholm` writes).  covariation: see _final.
    The first decode of every family's final alignment is one Context.consensus_structures call over all of them.
    row_structures: each Result also gets .row_ss, per printed row the structure of that row alone (a uint32 array over its
    residues, NONE for unpaired): the one-row alignment of its sequence decoded from the base-pairing store this phase read,
    at the threshold of the common structure -- after the consistency transform that store holds what the row's homologs
    say; and .row_ss_str, those structures laid into the rows' columns (stockholm.row_ss_str), which
    the Stockholm block carries as `#=GR <name> SS` lines.  All rows of all families are one consensus_structures call."""
    import time
    covariation = cov_options(covariation)
    nf = len(fams)
    results = []
    trees = []
    aln = {}  # (family, node) -> (global sequence indices, mask)
    pending = []
    for f, fm in enumerate(fams):
        score, left, right = fm["tree"]
        n = len(fm["seqs"])
        res = Result()
        res.sim = fm["sim"]
        res.tree = (score, left, right)
        res.tree_line = tree_string(score, left, right, fm["names"])
        res.dd_log = {}
        res.dd_dims = {}  # node -> (columns of the left, of the right alignment); resident-node mode only
        res.levels = 0
        res.rounds = []  # resident-node mode: (seconds, [(node, columns left, columns right), ...]) per round (diagnostics)
        results.append(res)
        trees.append((left, right))
        for i in range(n):
            aln[(f, i)] = (np.array([fm["first"] + i], np.uint32), np.ones((1, len(fm["seqs"][i])), np.uint8))
        pending += [(f, i) for i in range(n, 2 * n - 1)]
    done = set(aln)

    def key(f, i):  # node names in the diagnostics and keys of the schedule: the plain node index for one family
        return i if nf == 1 else (f, i)

    def node_input(f, i):
        left, right = trees[f]
        a1, a2 = aln[(f, left[i])], aln[(f, right[i])]
        if bp_update and i == 2 * len(fams[f]["seqs"]) - 2:
            # --bp-update: the top call of the recursion (DAFS::align(ss, aln, root), dafs.cpp:1518-1537) re-estimates
            # both base-pairing matrices under the structure decoded from their averages (:919-934)
            upd = []
            for s_idx, msk in (a1, a2):
                _, ss0, _ = ctx.consensus_structure(s_idx, msk, th_s)
                upd.append(ctx.update_basepairing(s_idx, msk, ss0))
            return (a1[0], a1[1], a2[0], a2[1], upd[0], upd[1])
        return (a1[0], a1[1], a2[0], a2[1])

    def take_ready():
        nonlocal pending
        ready = forest_ready(trees, pending, done)
        if ready and trace and not level_sync:
            print("open", [(key(f, i), aln[(f, trees[f][0][i])][1].shape, aln[(f, trees[f][1][i])][1].shape) for f, i in ready],
                  file=sys.stderr, flush=True)
        rs = set(ready)
        pending = [q for q in pending if q not in rs]
        return [(key(f, i), node_input(f, i)) for f, i in ready]

    def finish(k, o, dims):
        f, i = (0, k) if nf == 1 else k
        left, right = trees[f]
        aln[(f, i)] = project_alignment(aln[(f, left[i])], aln[(f, right[i])], o["z"])
        done.add((f, i))
        results[f].dd_log[i] = (o["iterations"], o["violated"], o["ncbp"], o["score"])
        if dims is not None:
            results[f].dd_dims[i] = dims
        del aln[(f, left[i])], aln[(f, right[i])]

    # progressive phase (_solve_nodes).  Only the alignment z of a node is consumed here (DAFS::align_alignments,
    # dafs.cpp:896-912), so nodes that have no consensus base pair to couple their subproblems need not run their two
    # folding DPs (dafs_dd_params doc)
    prm = capi.dd_params(w=w, eta0=eta0, th_a=th_a, th_s=th_s, t_max=t_max, force_iters=force_iters,
                         skip_uncoupled_folds=1 if skip_uncoupled_folds else 0)
    trace = os.environ.get("DAFS_PIPELINE_TRACE") == "1"  # node shapes on stderr as they are opened (diagnostics)
    levels, rounds, dd_memory, dd_demotions = _solve_nodes(ctx, prm, take_ready, finish, level_sync, slice_iters, round_us)
    if not level_sync:
        for res in results:
            res.dd_memory = dd_memory
            res.dd_demotions = dd_demotions
            res.skip_uncoupled_folds = bool(skip_uncoupled_folds)  # nodes without consensus pairs then carry no folding arrays
    t.append(time.perf_counter())
    th1 = th_s if th_s1 is None else th_s1
    roots = [aln[(f, 2 * len(fm["seqs"]) - 2)] for f, fm in enumerate(fams)]
    decoded = _decode(ctx, roots, th1)
    rows_ss = rows_level = rows_auto = [None] * nf
    if row_structures:
        lens = {fm["first"] + i: len(sq) for fm in fams for i, sq in enumerate(fm["seqs"])}
        rows_ss, rows_level, rows_auto = _row_structures(ctx, [sidx for sidx, _ in roots], lens, th1)
    finals = [_final_structure(ctx, sidx, mask, th1, bp_update1, ss) for (sidx, mask), (ss, *_) in zip(roots, decoded)]
    rls = ctx.alignment_reliabilities(roots, finals) if reliability else [None] * nf  # once every structure is final
    for f, (fm, res) in enumerate(zip(fams, results)):
        res.levels = levels
        res.rounds = rounds
        sidx, mask = roots[f]
        _final(ctx, res, fm["names"], fm["seqs"], fm["first"], sidx, mask, finals[f], rls[f], res.tree_line, None, covariation, rows_ss[f],
               identity, compare, phylogeny, decoded[f][1:], rows_level[f], rows_auto[f])
    t.append(time.perf_counter())
    # fold_launch: the folding is only started there; its kernels overlap `pair` and the first half of `pct_fold_tree`,
    # which also holds the wait for them
    seconds = dict(fold_launch=t[1] - t[0], pair=t[2] - t[1], pct_fold_tree=t[3] - t[2], progressive=t[4] - t[3], final=t[5] - t[4],
                   total=t[5] - t[0])
    for res in results:
        res.seconds = seconds
    if own:
        ctx.close()
    return results


def cov_options(covariation):
    """The covariation option of run / run_batch / add as a dict with shuffles, seed and e_max, or None for off.  The key
    null (one of capi.COV_NULLS; "tree" takes the default tree of the printed rows) is kept only where the caller gave it:
    without it the null is "shuffle".  The key tree (one of capi.COV_TREES, with null="tree" only; `dafs --cov-tree`) names
    that tree: "average", the default, or "nj", the neighbour-joining tree of the printed rows."""
    if covariation is None or covariation is False:
        return None
    opt = dict(shuffles=100, seed=1, e_max=0.05)
    if covariation is not True:
        unknown = set(covariation) - set(opt) - {"null", "tree"}
        if unknown:
            raise ValueError("covariation: unknown keys %s (shuffles, seed, e_max, null, tree)" % sorted(unknown))
        opt.update(covariation)
    if opt.get("null", "shuffle") not in capi.COV_NULLS:
        raise ValueError("covariation: unknown null %r (one of %s)" % (opt["null"], ", ".join(capi.COV_NULLS)))
    if "tree" in opt:  # --cov-tree: "average" is the library's default tree, "nj" the neighbour-joining tree of the rows
        if opt["tree"] not in capi.COV_TREES:
            raise ValueError(capi.phylogeny_refusal(capi.PHY_UNKNOWN_COV_TREE))
        if opt.get("null", "shuffle") != "tree":
            raise ValueError(capi.phylogeny_refusal(capi.PHY_COV_TREE_NEEDS_NULL))
    return opt


def _covariation(ctx, rows, ss, covariation):
    """Context.alignment_covariation under the options of cov_options, the options beside the arrays.  tree="nj": the tree null
    evolves along the neighbour-joining tree of the rows (Context.alignment_tree, model "jc")."""
    tree = None
    if covariation.get("tree") == "nj" and len(rows) >= 2:
        tree = ctx.alignment_tree(rows)[:2]
    cv = ctx.alignment_covariation(rows, ss, shuffles=covariation["shuffles"], seed=covariation["seed"], null=covariation.get("null", "shuffle"),
                                   tree=tree)
    cv.update(covariation)
    return cv


class Phylogeny:
    """Result of alignment_phylogeny: .model, .left, .right, .length (Context.alignment_tree) and .newick (capi.newick); with
    bootstrap replicates also .support (Context.alignment_bootstrap), .replicates, .seed and .support_table
    (capi.support_table), and .newick then carries the support in percent as the labels of the joins; with the transfer
    option also .transfer and .depth, .newick carries the transfer bootstrap expectation in percent
    and .support_table is capi.transfer_table's"""


class PhylogenyOption(str):
    """The model name of the phylogeny option as it travels through the drivers, with the bootstrap options beside it:
    .bootstrap (replicates, 0 for none), .seed and .transfer (the transfer bootstrap of DESIGN.md section 28)"""
    bootstrap, seed, transfer = 0, 12345, False


def phylogeny_option(phylogeny, bootstrap=0, seed=12345, transfer=False):
    """phylogeny_model with the bootstrap options of run / run_batch / add / describe / cluster checked and attached
    (DESIGN.md section 23): None for off, otherwise a PhylogenyOption.  Replicates without a tree are refused with the
    library's text, as the command line refuses --phylogeny-bootstrap without --phylogeny; so is the transfer option
    (section 28) without replicates."""
    model = phylogeny_model(phylogeny)
    if isinstance(model, PhylogenyOption):
        return model
    bootstrap = int(bootstrap or 0)
    if model is None:
        if bootstrap:
            raise ValueError(capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE))
        if transfer:
            raise ValueError(capi.transfer_refusal(capi.TRANSFER_NEEDS_REPLICATES))
        return None
    if not 0 <= bootstrap <= capi.BOOTSTRAP_MAX:
        raise ValueError(capi.bootstrap_refusal(capi.BOOT_COUNT))
    if transfer and not bootstrap:
        raise ValueError(capi.transfer_refusal(capi.TRANSFER_NEEDS_REPLICATES))
    out = PhylogenyOption(model)
    out.bootstrap, out.seed, out.transfer = bootstrap, int(seed) & 0xFFFFFFFFFFFFFFFF, bool(transfer)
    return out


def phylogeny_model(phylogeny):
    """The phylogeny option of run / run_batch / add / describe / cluster as a model name, or None for off (False, None).
    True is "jc"."""
    if phylogeny is None or phylogeny is False:
        return None
    if phylogeny is True:
        return "jc"
    if isinstance(phylogeny, PhylogenyOption):
        return phylogeny
    if phylogeny not in capi.NJ_MODELS:
        raise ValueError(capi.phylogeny_refusal(capi.PHY_UNKNOWN_MODEL))
    return phylogeny


def alignment_phylogeny(ctx, row_names, rows, model="jc"):
    """The neighbour-joining tree of an alignment's rows (`dafs --phylogeny OUT`): Context.alignment_tree
    over all columns under `model`, and the Newick line with the rows' Stockholm names, byte for byte the command line's.
    A model that is a PhylogenyOption with replicates (`--phylogeny-bootstrap B`) adds their support."""
    out = Phylogeny()
    out.model = str(model)
    out.left, out.right, out.length = ctx.alignment_tree(rows, model=out.model)
    replicates = getattr(model, "bootstrap", 0)
    if not replicates:
        out.newick = capi.newick(row_names, out.left, out.right, out.length)
        return out
    out.replicates, out.seed = replicates, model.seed
    if getattr(model, "transfer", False):
        out.support, out.transfer = ctx.alignment_bootstrap(rows, model=out.model, B=replicates, seed=model.seed, tree=(out.left, out.right),
                                                            transfer=True)
        out.depth = capi.split_depth(out.left, out.right)
        out.newick = capi.newick(row_names, out.left, out.right, out.length, transfer=out.transfer, depth=out.depth, replicates=replicates)
        out.support_table = capi.transfer_table(row_names, out.left, out.right, out.support, out.transfer, replicates, model.seed, out.model)
        return out
    out.support = ctx.alignment_bootstrap(rows, model=out.model, B=replicates, seed=model.seed, tree=(out.left, out.right))
    out.newick = capi.newick(row_names, out.left, out.right, out.length, support=out.support, replicates=replicates)
    out.support_table = capi.support_table(row_names, out.left, out.right, out.support, replicates, model.seed, out.model)
    return out


def _row_structures(ctx, sidx_per_alignment, lens, th):
    """Per alignment (its rows' global sequence indices) and per printed row (ascending index) the structure of that row's
    sequence alone from the context's current base-pairing store: one Context.consensus_structures call over all of them.
    lens: global sequence index -> length.  Returns (structures, levels, choices), each a list per alignment of one entry per
    row; the levels of an alignment are None under the plain decoder, and the choices (capi.AutoChoice: every row chooses its
    own thresholds) unless th is a capi.AutoThresholds."""
    printed = [np.sort(np.asarray(sidx, np.uint32), kind="stable") for sidx in sidx_per_alignment]
    flat = [int(x) for rows in printed for x in rows]
    got = _decode(ctx, [(np.array([x], np.uint32), np.ones((1, lens[x]), np.uint8)) for x in flat], th)
    out, levels, autos, k = [], [], [], 0
    for rows in printed:
        mine = got[k:k + len(rows)]
        out.append([ss for ss, *_ in mine])
        levels.append([level for _, level, _, _ in mine] if _by_level(th) else None)
        autos.append([auto for *_, auto in mine] if isinstance(th, capi.AutoThresholds) else None)
        k += len(rows)
    return out, levels, autos


def _final_structure(ctx, sidx, mask, th1, bp_update1, ss):
    """The common structure of a final alignment (sidx: global sequence index per row, mask) from its first decode ss (a
    batched Context.consensus_structures call)"""
    if bp_update1:  # :1863-1869: decode, re-estimate under that structure, decode again
        _, ss = ctx.nussinov(ctx.update_basepairing(sidx, mask, ss), None, th1)
    return ss


def alignment_identity(ctx, rows, use=None):
    """How similar the rows of an alignment are: Context.alignment_identity with its matrices, plus
    .weights (Context.alignment_weights), .pid (the identity to the nearest row, NaN for a single row) and .summary (average,
    minimum, maximum pid over all pairs; capi.identity_summary).  use: the columns that count (None: all)."""
    if len(rows) > 32768:
        raise ValueError(capi.alistat_refusal(capi.TOO_MANY_ROWS))
    ident = ctx.alignment_identity(rows, use=use, matrix=True)
    ident.weights = ctx.alignment_weights(rows, use=use)
    ident.pid = ident.pid_nearest
    ident.summary = capi.identity_summary(ident.ident, ident.res)
    ident.columns = len(rows[0])
    return ident


def identity_tsv(row_names, identity):
    """The table of `dafs --identity OUT` for one alignment (dafs_host_identity_table): the line "# rows n columns len average
    A min B max C", then per row "r<TAB>name<TAB>residues<TAB>weight<TAB>nearest<TAB>nearest_name<TAB>pid" with 1-based
    indices and the floats as %.9g.  row_names: the rows' Stockholm names."""
    row_names = list(row_names)
    n = len(identity.res)
    if len(row_names) != n:
        raise ValueError("identity_tsv: one name per row")
    arrs = [np.ascontiguousarray(a, t) for a, t in ((identity.res, np.uint32), (identity.weights, np.float64), (identity.nearest, np.uint32),
                                                    (identity.nearest_ident, np.uint32), (identity.nearest_den, np.uint32),
                                                    (identity.summary, np.float64))]
    return capi.host_text(capi._identity_table, n, int(identity.columns), capi.c_strings(row_names), *[a.ctypes.data for a in arrs])


def identity_matrix_tsv(row_names, identity):
    """The table of `dafs --identity-matrix OUT` (dafs_host_identity_matrix_table): per pair r < s the line
    r, s, name_r, name_s, ident, aligned, den, pid, tab-separated"""
    row_names = list(row_names)
    n = len(identity.res)
    if len(row_names) != n:
        raise ValueError("identity_matrix_tsv: one name per row")
    arrs = [np.ascontiguousarray(a, np.uint32) for a in (identity.res, identity.ident, identity.aligned)]
    return capi.host_text(capi._identity_matrix_table, n, capi.c_strings(row_names), *[a.ctypes.data for a in arrs])


def describe(names, rows, ss=None, ctx=None, identity=True, covariation=False, compare=None, pp=None, phylogeny=False,
             phylogeny_bootstrap=0, phylogeny_seed=12345, level=None, phylogeny_transfer=False):
    """The alignment-only statistics of a finished alignment (`dafs --describe ALIGNMENT`): nothing is
    aligned.  names / rows / ss: as stockholm.read_seed_structure returns them (ss None: no structure).  Returns a Result with
    .rows, .row_names (stockholm.names), .ss and, as asked, .identity (alignment_identity over all columns) and .covariation
    (as run's).  compare (as run's): .compare, this alignment against the reference; pp: its PP rows (stockholm.read_seed_pp)
    for the comparison's PP part.  phylogeny, phylogeny_bootstrap, phylogeny_seed, phylogeny_transfer (as run's): .phylogeny.  level (with ss, both
    as stockholm.read_seed_knots returns them; `dafs --describe --knots`): the levels of a structure whose
    pairs may cross -> .ss_level and .ss_str, the brackets of capi.make_brackets_levels, which `dafs` prints after a
    ">SS_cons" line; the statistics read the merged ss."""
    covariation = cov_options(covariation)
    phylogeny = phylogeny_option(phylogeny, phylogeny_bootstrap, phylogeny_seed, phylogeny_transfer)
    names, rows = stockholm.clean_seed(names, rows)
    res = Result()
    res.rows, res.row_names = rows, stockholm.names(names)
    res.ss = np.full(len(rows[0]), NONE, np.uint32) if ss is None else np.ascontiguousarray(ss, np.uint32)
    if len(res.ss) != len(rows[0]):
        raise ValueError("pipeline.describe: the structure needs one entry per column")
    if level is not None:
        res.ss_level = np.ascontiguousarray(level, np.uint8)
        if ss is None or len(res.ss_level) != len(res.ss):
            raise ValueError("pipeline.describe: level needs ss and one entry per column")
        res.ss_str = capi.make_brackets_levels(res.ss, res.ss_level)
    own = ctx is None
    if own:
        ctx = capi.Context(0)
    try:
        if identity:
            res.identity = alignment_identity(ctx, rows)
        if phylogeny:
            res.phylogeny = alignment_phylogeny(ctx, res.row_names, rows, phylogeny)
        if covariation:
            res.covariation = _covariation(ctx, rows, res.ss, covariation)
        if compare is not None:
            res.compare = compare_result(ctx, compare, res.row_names, rows, None if ss is None else res.ss, pp=pp)
    finally:
        if own:
            ctx.close()
    return res


def compare(ref_names, ref_rows, names, rows, ref_ss=None, ss=None, use_ref=None, use_test=None, pp=None, ctx=None, matrix=True):
    """How far the alignment (names, rows) agrees with the reference (ref_names, ref_rows) of the same sequences (DESIGN.md
    section 19; `dafs --compare`).  The compared rows are the names (first words) present in both, in the reference's order
    (capi.compare_match); both alignments are cut to them and keep their columns.  ref_ss / ss: the two structures, both or
    the structure part is left out; use_ref / use_test: the aligned columns; pp: per row of `rows` its PP characters, or
    None.  Returns (result, table, columns_table, matrix_table): the Context.alignment_compare result with .row_names,
    .only_ref and .only_test, and the texts of --compare, --compare-columns and --compare-matrix (None without matrix)."""
    ref_names, names = list(ref_names), list(names)
    if len(ref_names) != len(ref_rows) or len(names) != len(rows):
        raise ValueError("pipeline.compare: one name per row")
    ref_row, test_row = capi.compare_match(ref_names, names)
    n = len(ref_row)
    if matrix and n > 16384:
        raise ValueError(capi.compare_refusal(capi.CMP_TOO_MANY_ROWS))
    both = ref_ss is not None and ss is not None
    own = ctx is None
    if own:
        ctx = capi.Context(0)
    try:
        res = ctx.alignment_compare([ref_rows[i] for i in ref_row], [rows[i] for i in test_row], use_ref=use_ref, use_test=use_test,
                                    ss_ref=ref_ss if both else None, ss_test=ss if both else None,
                                    pp=None if pp is None else capi.encode_pp([pp[i] for i in test_row]), matrix=matrix)
    finally:
        if own:
            ctx.close()
    res.row_names = [(ref_names[i].split() or [""])[0] for i in ref_row]
    res.only_ref, res.only_test = len(ref_names) - n, len(names) - n
    u64 = lambda a: np.ascontiguousarray(a, np.uint64)  # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    names_c = capi.c_strings(res.row_names)
    total, tc = u64([res.total_shared, res.total_refp, res.total_testp]), u64([res.tc_reproduced, res.tc_columns])
    ss_arrs = [u64(a) for a in (res.tp, res.nref, res.ntest)] if both else [None] * 3
    pp_count = u64(np.concatenate([res.pp_residues, res.pp_ref, res.pp_shared])) if pp is not None else None
    table = capi.host_text(capi._compare_table, n, names_c, res.only_ref, res.only_test, len(res.k), len(res.m), res.residues.ctypes.data,
                           res.shared.ctypes.data, res.refp.ctypes.data, res.testp.ctypes.data, total.ctypes.data, tc.ctypes.data,
                           *[ptr(a) for a in ss_arrs], ptr(pp_count))
    rep8 = np.ascontiguousarray(res.reproduced, np.uint8)
    columns = capi.host_text(capi._compare_columns_table, len(res.k), res.k.ctypes.data, res.colref.ctypes.data, res.colshared.ctypes.data,
                             rep8.ctypes.data)
    pairs = None
    if matrix:
        pairs = capi.host_text(capi._compare_matrix_table, n, names_c, res.pair_shared.ctypes.data, res.pair_refp.ctypes.data,
                               res.pair_testp.ctypes.data)
    return res, table, columns, pairs


def compare_result(ctx, reference, row_names, rows, ss, use_test=None, pp=None):
    """compare() for a driver's compare=(ref_names, ref_rows[, ref_ss]) option: the result with the three texts as .table,
    .columns_table and .matrix_table"""
    if len(reference) not in (2, 3):
        raise ValueError("compare: the reference is (ref_names, ref_rows) or (ref_names, ref_rows, ref_ss)")
    ref_ss = reference[2] if len(reference) == 3 else None
    res, table, columns, pairs = compare(reference[0], reference[1], row_names, rows, ref_ss, ss, use_test=use_test, pp=pp, ctx=ctx,
                                         matrix=len(rows) <= 16384)
    res.table, res.columns_table, res.matrix_table = table, columns, pairs
    return res


def _final(ctx, res, names, seqs, first, sidx, mask, ss, rl, tree_line, rf=None, covariation=None, row_ss=None, identity=False, compare=None,
           phylogeny=False, levels=None, row_level=None, row_auto=None):
    """The output of a final alignment (sidx: global sequence index per row, mask) with its common structure ss
    (_final_structure), into res: .ss, .ss_str, .rows, .output and, with rl, .reliability and .stockholm.  names / seqs: the
    family's, its first sequence at global index `first`.  rl: the alignment's dict of Context.alignment_reliabilities for
    (sidx, mask, ss), made by the caller in one call over all its alignments, or None for no annotation.  tree_line None: no
    tree line (pipeline.add); rf: the RF line of the Stockholm block.  covariation (cov_options): .covariation, the dict of
    Context.alignment_covariation on the printed rows and structure with the options' shuffles, seed
    and e_max beside the arrays; the Stockholm block then carries a `#=GC cov_SS_cons` line.  row_ss: per printed row its own structure (_row_structures) -> .row_ss, .row_ss_str
    and the `#=GR <name> SS` lines of the Stockholm block.  identity: .identity, alignment_identity of the printed rows in
    printed order over all columns, and .row_names, their Stockholm names; the Stockholm block then carries the `#=GS <name> WT` lines.
    compare: a reference (run's compare) -> .compare, the printed rows and ss against it (compare_result), and .row_names.
    phylogeny: a model -> .phylogeny (alignment_phylogeny of the printed rows), and .row_names.  levels: (level, scores) of a
    structure decoded level by level (_decode), or None / (None, None) -> .ss_level, .ss_scores, and .ss_str with the bracket
    kind of each pair's level; row_level: the same per printed row for row_ss.  levels may carry a third entry, the
    capi.AutoChoice of thresholds chosen automatically -> .ss_auto; row_auto: per printed row -> .row_ss_auto."""
    phylogeny = phylogeny_model(phylogeny)
    res.ss = ss
    res.root = (sidx, mask)  # the alignment as it was decoded: the rows in this order (the average depends on it)
    if levels is None or levels[0] is None:
        res.ss_str = capi.make_brackets(ss)
    else:
        res.ss_level, res.ss_scores = levels[:2]
        res.ss_str = capi.make_brackets_levels(ss, res.ss_level)
        if len(levels) > 2 and levels[2] is not None:
            res.ss_auto = levels[2]
    order = np.argsort(sidx, kind="stable")  # std::sort(aln) :1876
    lines = ([] if tree_line is None else [tree_line]) + [">SS_cons", res.ss_str]
    res.rows = []
    for r in order:
        row_bytes = np.full(mask.shape[1], ord("-"), np.uint8)
        local = int(sidx[r]) - first
        row_bytes[mask[r].astype(bool)] = np.frombuffer(seqs[local].encode("latin-1"), np.uint8)  # residues into their columns
        row = row_bytes.tobytes().decode("latin-1")
        res.rows.append(row)
        lines += ["> " + names[local], row]
    res.output = "\n".join(lines) + "\n"
    if row_ss is not None:
        res.row_ss = row_ss
        if row_level is None:
            res.row_ss_str = [stockholm.row_ss_str(row, x) for row, x in zip(res.rows, row_ss)]
        else:
            res.row_ss_level = row_level
            res.row_ss_str = [stockholm.row_ss_str(row, x, lv) for row, x, lv in zip(res.rows, row_ss, row_level)]
        if row_auto is not None:
            res.row_ss_auto = row_auto
    cov_chars = None
    if covariation:
        cv = _covariation(ctx, res.rows, ss, covariation)
        res.covariation = cv
        cov_chars = stockholm.cov_ss_cons(ss, cv["pair_e"], cv["e_max"])
    if identity or compare is not None or phylogeny:
        sto_names = stockholm.names(names)
        res.row_names = [sto_names[int(sidx[r]) - first] for r in order]
    if identity:
        res.identity = alignment_identity(ctx, res.rows)
    if phylogeny:
        res.phylogeny = alignment_phylogeny(ctx, res.row_names, res.rows, phylogeny)
    if compare is not None:
        res.compare = compare_result(ctx, compare, res.row_names, res.rows, ss)
    if rl is not None:
        rl = dict(rl)
        cuts = np.cumsum([len(seqs[int(s) - first]) for s in sidx])[:-1]
        per_row = np.split(rl["residue"], cuts)  # rows in the order of sidx
        rl["residue"] = [per_row[r] for r in order]
        res.reliability = rl
        sto_names = stockholm.names(names)
        res.stockholm = stockholm.block(tree_line, [sto_names[int(sidx[r]) - first] for r in order], res.rows, rl["residue"],
                                        rl["col"], res.ss_str, rf, cov_chars, None if row_ss is None else res.row_ss_str,
                                        res.identity.weights if identity else None)


def _seed_structure(seed_ss, seed_mask, seed_seqs, th_s1, bp_update1, who, seed_level=None):
    """The checks of a seed structure (seed_ss over the seed's cleaned columns) and the folding constraint it puts on every
    seed row (capi.row_constraint).  Returns (seed_ss as uint32, None, constraints).  seed_level: the
    pairs' levels, checked too (0xFF exactly at the unpaired columns, equal at both columns of a pair, below capi.MAX_LEVELS,
    every level nested in itself); returns (seed_ss, seed_level as uint8, constraints), every row's entry then the list of its
    per-level constraints (capi.row_constraint_levels)."""
    ss = np.ascontiguousarray(seed_ss, np.uint32).reshape(-1)
    C = seed_mask.shape[1]
    if len(ss) != C:
        raise ValueError("%s: seed_ss has %d entries, the seed has %d columns" % (who, len(ss), C))
    if bp_update1 or th_s1 is not None:
        raise ValueError("%s: with seed_ss nothing is decoded: bp_update1 and th_s1 cannot be combined with it" % who)
    used = np.zeros(C, bool)
    for c in range(C):
        p = int(ss[c])
        if p == NONE:
            continue
        if p <= c or p >= C or used[c] or used[p]:
            raise ValueError("%s: seed_ss is no structure over the seed's columns (column %d)" % (who, c))
        used[c] = used[p] = True
    if seed_level is None:
        return ss, None, [capi.row_constraint(seed_mask[r], ss, seed_seqs[r]) for r in range(len(seed_seqs))]
    level = np.ascontiguousarray(seed_level, np.uint8).reshape(-1)
    if len(level) != C:
        raise ValueError("%s: seed_level has %d entries, the seed has %d columns" % (who, len(level), C))
    open_at = [[] for _ in range(capi.MAX_LEVELS)]  # per level the right columns of its open pairs
    for c in range(C):
        lv = int(level[c])
        if not used[c]:
            if lv != 0xFF:
                raise ValueError("%s: seed_level gives the unpaired column %d a level" % (who, c))
            continue
        if lv >= capi.MAX_LEVELS:
            raise ValueError("%s: seed_level holds %d at the paired column %d; the levels are 0..%d" % (who, lv, c, capi.MAX_LEVELS - 1))
        if ss[c] != NONE:
            if int(level[ss[c]]) != lv:
                raise ValueError("%s: seed_level differs at the two columns of the pair at column %d" % (who, c))
            open_at[lv].append(int(ss[c]))
        elif not open_at[lv] or open_at[lv].pop() != c:
            raise ValueError("%s: the pairs of level %d of seed_level cross (column %d)" % (who, lv, c))
    K = int(level[used].max()) + 1 if used.any() else 1
    return ss, level, [capi.row_constraint_levels(seed_mask[r], ss, level, K, seed_seqs[r]) for r in range(len(seed_seqs))]


def carry_structure(seed_ss, seed_col, width, seed_level=None):
    """The seed's structure in the merged columns: ss_m[seed_col[c]] = seed_col[seed_ss[c]], insert columns unpaired.  seed_level:
    the pairs' levels travel with their columns (0xFF at insert columns); returns (ss_m, level_m)."""
    ss_m = np.full(width, NONE, np.uint32)
    paired = np.flatnonzero(seed_ss != NONE)
    ss_m[seed_col[paired]] = seed_col[seed_ss[paired]]
    if seed_level is None:
        return ss_m
    level_m = np.full(width, 0xFF, np.uint8)
    level_m[seed_col] = seed_level
    return ss_m, level_m


def _printed_support(sup, sidx):
    """one alignment's Context.structure_support in the order of its printed rows (ascending sequence index)"""
    order = np.argsort(sidx, kind="stable")
    return {k: v[order] for k, v in sup.items()}


def add(seed_names, seed_rows, names, seqs, ctx=None, w=4.0, eta0=0.5, t_max=600, w_pct_a=0.25, w_pct_s=0.25, th_a=0.01,
        th_s=0.2, th_s1=None, align_model=capi.ALIGN_PROBCONS, force_iters=0, slice_iters=None, skip_uncoupled_folds=True,
        round_us=None, w_pct_f=0.0, bp_update1=False, reliability=False, covariation=False, row_structures=False, seed_ss=None,
        decoder="Nussinov", seed_level=None,
        identity=False, compare=None, phylogeny=False, phylogeny_bootstrap=0, phylogeny_seed=12345, phylogeny_transfer=False):
    """Add new sequences to a fixed seed alignment without changing its columns (`dafs --seed`).
    seed_names / seed_rows: the seed's rows (letters and '.' / '-' gaps; stockholm.read_seed reads a file), checked and
    without their all-gap columns (stockholm.clean_seed).  names / seqs: the new sequences.  The options are run()'s.

    The context holds the m seed sequences and then the k new ones; phase 1 is a normal run's over all of them.  One node per
    new sequence j (its leaf against the seed), all k through the resident-node rounds together; the merge is
    capi.merge_added (dafs_host_merge_added); the structure is decoded over the rows new sequences then seed rows.
    Returns a Result: .output (a normal run's format without the tree line: rows in context order), .rows, .ss, .ss_str,
    .z (per new sequence its column map into the seed), .rf (per merged column True for a seed column), .dd_log
    ({j: (iterations, violated, ncbp, score)}), .dd_memory, .seconds; with reliability, .reliability and .stockholm (no CC
    line, a `#=GC RF` line); with covariation (as in run), .covariation; with row_structures (as in run), .row_ss and
    .row_ss_str; with identity (as in run), .identity; with compare (as in run), .compare; with phylogeny (as in run),
    .phylogeny.

    seed_ss (`dafs --seed-structure`): the seed's consensus structure over its cleaned columns
    (stockholm.read_seed_structure), fixed like the columns.  The seed rows are folded under the constraints it puts on them
    (capi.row_constraint), the new sequences free; nothing is decoded: the output's structure is the seed's carried into the
    merged columns, insert columns unpaired, and the annotations see it.  The Result gains .support: per printed row, both,
    canonical, half and expected of Context.structure_support.

    seed_level (`dafs --seed-structure --knots`; only with seed_ss): the levels of seed_ss's pairs
    (stockholm.read_seed_knots), whose pairs may then cross between levels.  Every seed row is folded once per level that
    forces a pair in it (capi.row_constraint_levels; Context.fold_begin merges the folds); the Result gains .ss_level, and
    .ss_str and the Stockholm SS_cons print "()", "[]", "{}", "<>" for levels 0..3.  .support reads the merged structure."""
    import time
    th_s1 = decoder_option(decoder, th_s, th_s1, bp_update1, seed_ss, "pipeline.add")  # decoder: as in run()
    if seed_level is not None and seed_ss is None:
        raise ValueError("pipeline.add: seed_level gives the levels of seed_ss and needs it")
    covariation = cov_options(covariation)
    phylogeny = phylogeny_option(phylogeny, phylogeny_bootstrap, phylogeny_seed, phylogeny_transfer)
    seed_names, seed_rows = stockholm.clean_seed(seed_names, seed_rows)
    names, seqs = list(names), list(seqs)
    if not seqs or len(names) != len(seqs):
        raise ValueError("pipeline.add: at least one new sequence and one name per sequence")
    m, k = len(seed_rows), len(seqs)
    seed_seqs = [r.replace("-", "") for r in seed_rows]
    seed_mask = np.array([[ch != "-" for ch in r] for r in seed_rows], np.uint8)
    all_names, all_seqs = seed_names + names, seed_seqs + seqs
    constraints = None
    if seed_ss is not None:
        seed_ss, seed_level, constraints = _seed_structure(seed_ss, seed_mask, seed_seqs, th_s1, bp_update1, "pipeline.add", seed_level)
        constraints += [None] * k
    own = ctx is None
    if own:
        ctx = capi.Context(0)
    try:
        t = [time.perf_counter()]
        _phase1_local(ctx, all_seqs, None, None, align_model, th_a, w_pct_a, w_pct_s, t, w_pct_f, constraints=constraints)
        t.append(time.perf_counter())
        prm = capi.dd_params(w=w, eta0=eta0, th_a=th_a, th_s=th_s, t_max=t_max, force_iters=force_iters,
                             skip_uncoupled_folds=1 if skip_uncoupled_folds else 0)
        seed_idx = np.arange(m, dtype=np.uint32)
        new = [(j, (np.array([m + j], np.uint32), np.ones((1, len(seqs[j])), np.uint8), seed_idx, seed_mask)) for j in range(k)]
        outs = [None] * k
        batches = iter([new])  # every node is ready in the first round, none later

        def finish(j, o, dims):
            outs[j] = o
        _, _, dd_memory, _ = _solve_nodes(ctx, prm, lambda: next(batches, []), finish, slice_iters=slice_iters, round_us=round_us)
        t.append(time.perf_counter())
        # the merge, then the rows in the order new sequences, seed rows (the sidx of a run that joins a leaf last)
        seed_col, res_col, width = capi.merge_added(seed_mask.shape[1], [o["z"] for o in outs])
        mask = np.zeros((m + k, width), np.uint8)
        mask[:m, seed_col] = seed_mask
        for j in range(k):
            mask[m + j, res_col[j]] = 1
        rf = np.zeros(width, bool)
        rf[seed_col] = True
        sidx = np.concatenate([np.arange(m, m + k), np.arange(m)]).astype(np.uint32)
        res = Result()
        res.z = [o["z"] for o in outs]
        res.rf = rf
        res.dd_log = {j: (o["iterations"], o["violated"], o["ncbp"], o["score"]) for j, o in enumerate(outs)}
        res.dd_memory = dd_memory
        th1 = th_s if th_s1 is None else th_s1
        rows_mask = np.concatenate([mask[m:], mask[:m]])
        ss_m = None if seed_ss is None else carry_structure(seed_ss, seed_col, width)
        levels = None
        if seed_level is not None:
            levels = (carry_structure(seed_ss, seed_col, width, seed_level)[1], None)
        if ss_m is not None:
            res.support = _printed_support(ctx.structure_support([(sidx, rows_mask)], [ss_m])[0], sidx)
        elif _by_level(th1):  # the batched call with one alignment
            ss_m, *levels = _decode(ctx, [(sidx, rows_mask)], th1)[0]
        else:
            ss_m = _final_structure(ctx, sidx, rows_mask, th1, bp_update1, ctx.consensus_structure(sidx, rows_mask, th1)[1])
        rl = ctx.alignment_reliability(sidx, rows_mask, ss_m) if reliability else None
        row_ss, row_level, row_auto = None, None, None
        if row_structures:
            row_ss, row_level, row_auto = (x[0] for x in _row_structures(ctx, [sidx], dict(enumerate(map(len, all_seqs))), th1))
        _final(ctx, res, all_names, all_seqs, 0, sidx, rows_mask, ss_m, rl, None, rf, covariation, row_ss, identity, compare, phylogeny,
               levels, row_level, row_auto)
        t.append(time.perf_counter())
        res.seconds = dict(phase1=t[3] - t[0], nodes=t[4] - t[3], final=t[5] - t[4], total=t[5] - t[0])
    finally:
        if own:
            ctx.close()
    return res


def family_bytes(lens):
    """Device memory one family takes in phase 1, estimated from the stores' sizes (bytes; dafs_host_family_bytes states what
    is counted).  Not counted: the folding kernels' workspaces and the resident nodes of the progressive phase, which hold
    only the open nodes (tools/time_batch.py reports their measured peak)."""
    lens = np.ascontiguousarray([int(x) for x in lens], np.uint32)
    return int(capi._family_bytes(len(lens), lens.ctypes.data))


def pack_families(sizes, max_bytes):
    """Sub-batches of the families (greedy, in input order; dafs_host_pack_greedy) whose estimated sizes add up to at most
    max_bytes each; a family over the budget runs alone.  Returns lists of family indices."""
    sizes = np.ascontiguousarray([int(b) for b in sizes], np.uint64)
    group = np.zeros(max(len(sizes), 1), np.uint32)
    capi.check(capi._pack_greedy(len(sizes), sizes.ctypes.data, int(max_bytes), group.ctypes.data))
    out = []
    for k in range(len(sizes)):
        if group[k] == len(out):
            out.append([])
        out[-1].append(k)
    return out


DEFAULT_BATCH_BYTES = int(capi._batch_bytes())  # per sub-batch or chunk: the library's choice (dafs_host_batch_bytes)


def run_batch(families, ctx=None, max_bytes=None, **kw):
    """Align many independent families in one context, sharing every device launch between them.  families: a list of
    (names, seqs).  kw: the options of run() except mp / bp / shard.  Returns one Result per family, in input order, each
    with the .output, .dd_log and .sim a separate run() of that family gives.  The families are packed greedily, in input
    order, into sub-batches under max_bytes of estimated device memory (family_bytes; default DEFAULT_BATCH_BYTES); phase 1
    runs once per sub-batch over the whole sub-batch, the guide trees are built per family and the progressive phase walks
    their forest."""
    import time
    for k in ("mp", "bp", "shard"):
        if k in kw:
            raise ValueError("pipeline.run_batch: %s is a single-family option (use run)" % k)
    if kw.get("level_sync") and kw.get("bp_update"):
        raise ValueError("pipeline.run_batch: bp_update needs the resident-node schedule (level_sync=False)")
    opts = {k: p.default for k, p in inspect.signature(run).parameters.items() if k not in ("names", "seqs", "ctx", "bp", "mp", "shard")}
    unknown = set(kw) - set(opts)
    if unknown:
        raise TypeError("pipeline.run_batch: unknown options %s" % sorted(unknown))
    opts.update(kw)
    opts["th_s1"] = decoder_option(opts["decoder"], opts["th_s"], opts["th_s1"], opts["bp_update1"], None, "pipeline.run_batch")
    opts["phylogeny"] = phylogeny_option(opts["phylogeny"], opts["phylogeny_bootstrap"], opts["phylogeny_seed"], opts["phylogeny_transfer"])
    families = [(list(nm), list(sq)) for nm, sq in families]
    for nm, sq in families:
        if not sq or len(nm) != len(sq):
            raise ValueError("pipeline.run_batch: every family needs at least one sequence and one name per sequence")
    budget = DEFAULT_BATCH_BYTES if max_bytes is None else int(max_bytes)
    groups = pack_families([family_bytes([len(s) for s in sq]) for _, sq in families], budget)
    own = ctx is None
    if own:
        ctx = capi.Context(0)
    out = [None] * len(families)
    try:
        for grp in groups:
            t = [time.perf_counter()]
            seqs, first = [], [0]
            for k in grp:
                seqs += families[k][1]
                first.append(len(seqs))
            sims = _phase1_local(ctx, seqs, None, None, opts["align_model"], opts["th_a"], opts["w_pct_a"], opts["w_pct_s"], t,
                                 opts["w_pct_f"], first)
            fams = []
            for j, k in enumerate(grp):
                fams.append(dict(names=families[k][0], seqs=families[k][1], first=first[j], sim=sims[j], tree=capi.build_tree(sims[j])))
            t.append(time.perf_counter())
            res = _phase2_forest(ctx, False, fams, t, opts["w"], opts["eta0"], opts["t_max"], opts["th_a"], opts["th_s"], opts["th_s1"],
                                 opts["force_iters"], opts["level_sync"], opts["slice_iters"], opts["skip_uncoupled_folds"], opts["round_us"],
                                 opts["bp_update"], opts["bp_update1"], opts["reliability"], opts["covariation"], opts["row_structures"],
                                 opts["identity"], None, opts["phylogeny"])
            for k, r in zip(grp, res):
                out[k] = r
    finally:
        if own:
            ctx.close()
    return out


# ------------------------------------------------------------------------------------------------ all-against-all pairs
def node_bytes(l1, l2):
    """Device memory of one resident node of l1 x l2 columns (bytes; dafs_host_node_bytes), the bound
    test_configs_gpu._node_bytes_bound states from capi_dd.cpp's nodes_open, folding arrays included."""
    return int(capi._node_bytes(int(l1), int(l2)))


def pair_bytes(l1, l2):
    """Device memory of one two-sequence family of a pairwise run: its phase-1 stores (family_bytes) and its root node, which
    is resident for the whole progressive phase of the chunk (every pair's one node opens in the first round)."""
    return family_bytes([l1, l2]) + node_bytes(l1, l2)


def all_pairs(n):
    """every pair (x, y), x < y < n, in row-major order"""
    return [(x, y) for x in range(n) for y in range(x + 1, n)]


def check_pairs(n, pairs):
    """The pair list of a pairwise run over n sequences as a list of (x, y) ints (all_pairs(n) for None); ValueError for
    n < 2, a pair with x >= y, an index out of range or a repeated pair."""
    if n < 2:
        raise ValueError("pipeline.pairwise: at least two sequences")
    if pairs is None:
        return all_pairs(n)
    out, seen = [], set()
    for pr in pairs:
        x, y = (int(v) for v in pr)
        if not 0 <= x < y < n:
            raise ValueError("pipeline.pairwise: pair (%d, %d) needs 0 <= x < y < %d" % (x, y, n))
        if (x, y) in seen:
            raise ValueError("pipeline.pairwise: pair (%d, %d) is repeated" % (x, y))
        seen.add((x, y))
        out.append((x, y))
    if not out:
        raise ValueError("pipeline.pairwise: the pair list is empty")
    return out


def pair_chunks(lens, pairs, max_bytes):
    """The pairs (indices into `pairs`) in chunks of at most max_bytes of estimated device memory each (pair_bytes), greedy
    in pair order; a pair over the budget runs alone."""
    return pack_families([pair_bytes(lens[x], lens[y]) for x, y in pairs], max_bytes)


def pairwise_scores_tsv(names, pairs, sim, score, iterations):
    """The table of `dafs --pairwise FILE --pairwise-scores OUT` (dafs_host_pairwise_table): per pair, in pair order,
    "i<TAB>j<TAB>name_i<TAB>name_j<TAB>sim<TAB>score<TAB>iterations" with 1-based i, j and the floats as %.9g.  sim, score,
    iterations: N x N, as pipeline.pairwise returns them."""
    names = list(names)
    xy = np.ascontiguousarray(np.array([(int(x), int(y)) for x, y in pairs], np.uint32).reshape(-1, 2).T)
    per_pair = [np.ascontiguousarray(np.asarray(a)[xy[0], xy[1]], t) for a, t in ((sim, np.float64), (score, np.float64), (iterations, np.int64))]
    return capi.host_text(capi._pairwise_table, xy.shape[1], xy[0].ctypes.data, xy[1].ctypes.data, len(names), capi.c_strings(names),
                          *[a.ctypes.data for a in per_pair])


class Pairwise:
    pass


COV_TABLE_E_MAX = 0.05  # the cut of the table's `other` pairs: fixed in the library, as on the command line (e_max moves cov_SS_cons only)


def covariation_tsv(result):
    """The table of `dafs --covariation OUT` for one result with .covariation (dafs_host_covariation_table): one line
    "c1<TAB>c2<TAB>kind<TAB>S<TAB>E<TAB>rows<TAB>canonical<TAB>types" per pair, columns 1-based, floats as %.9g.  First every
    consensus pair by ascending left column (kind ss); then every distinct pair {c, best(c)} that is no consensus pair and has
    E <= 0.05 (COV_TABLE_E_MAX, whatever the result's e_max), ordered by (c1, c2) (kind other), its counts taken from the rows."""
    cv = result.covariation
    code = capi.encode_alignment(result.rows)
    ss = np.ascontiguousarray(result.ss, np.uint32)
    arrs = [np.ascontiguousarray(cv[k], t) for k, t in (("best", np.uint32), ("best_score", np.float64), ("best_e", np.float64),
                                                         ("pair_score", np.float64), ("pair_e", np.float64), ("pair_rows", np.uint32),
                                                         ("pair_canonical", np.uint32), ("pair_types", np.uint32))]
    if any(a.shape != (code.shape[1],) for a in [ss] + arrs):
        raise ValueError("covariation_tsv: the structure and every array need one entry per column")
    return capi.host_text(capi._covariation_table, code.shape[0], code.shape[1], code.ctypes.data, ss.ctypes.data, *[a.ctypes.data for a in arrs])


def pairwise(names, seqs, pairs=None, ctx=None, max_bytes=None, **opts):
    """All pairwise structural alignments of a set of sequences (`dafs --pairwise`).  pairs: (x, y)
    with x < y, default every pair in row-major order.  opts: the options of run() except mp / bp / shard.  Each pair's
    Result is, bit for bit, what run([names[x], names[y]], [seqs[x], seqs[y]], **opts) gives (.output, .dd_log, .ss, .rows,
    .sim and, with reliability, .reliability / .stockholm; with row_structures, .row_ss / .row_ss_str from the pair's stores).

    Phase 1 (folds, all-pairs posteriors, no transforms) runs once over the N sequences in a source context of its own; the
    pairs go in chunks of at most max_bytes of estimated device memory (pair_chunks; default DEFAULT_BATCH_BYTES) through
    `ctx`: Context.pairs_from builds the chunk's two-sequence families on the device, then the transforms, the nodes of all
    of them in shared rounds (a two-leaf tree: its root alone) and the output.  Returns an object with .pairs, .results (one
    Result per pair, in pair order), .sim (N x N: the pair kernels' scores, Context.sim() of the N-sequence phase 1),
    .score and .iterations (N x N: the root node's final objective and iteration count, dd_log's 4th and 1st entries; NaN
    and -1 on the diagonal and for pairs not asked), .chunks (pair indices per chunk), .dd_memory (per chunk the nodes'
    (reserved, in use, peak) bytes) and .seconds (phase1, transforms, nodes, final, total)."""
    import time
    for k in ("mp", "bp", "shard"):
        if k in opts:
            raise ValueError("pipeline.pairwise: %s is a single-run option (use run)" % k)
    if opts.get("covariation"):
        raise ValueError("pipeline.pairwise: two rows carry no covariation; covariation is an option of run, run_batch and add")
    if opts.get("identity"):
        raise ValueError(capi.alistat_refusal(capi.NO_PAIRWISE))
    if opts.get("phylogeny"):
        raise ValueError(capi.phylogeny_refusal(capi.PHY_NO_PAIRWISE))
    if opts.get("phylogeny_bootstrap"):
        raise ValueError(capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE))
    if opts.get("phylogeny_transfer"):
        raise ValueError(capi.transfer_refusal(capi.TRANSFER_NEEDS_REPLICATES))
    if opts.get("compare") is not None:
        raise ValueError(capi.compare_refusal(capi.CMP_NO_PAIRWISE))
    if opts.get("level_sync") and opts.get("bp_update"):
        raise ValueError("pipeline.pairwise: bp_update needs the resident-node schedule (level_sync=False)")
    o = {k: p.default for k, p in inspect.signature(run).parameters.items() if k not in ("names", "seqs", "ctx", "bp", "mp", "shard")}
    unknown = set(opts) - set(o)
    if unknown:
        raise TypeError("pipeline.pairwise: unknown options %s" % sorted(unknown))
    o.update(opts)
    o["th_s1"] = decoder_option(o["decoder"], o["th_s"], o["th_s1"], o["bp_update1"], None, "pipeline.pairwise")
    names, seqs = list(names), list(seqs)
    if len(names) != len(seqs):
        raise ValueError("pipeline.pairwise: one name per sequence")
    n = len(seqs)
    pairs = check_pairs(n, pairs)
    chunks = pair_chunks([len(s) for s in seqs], pairs, DEFAULT_BATCH_BYTES if max_bytes is None else int(max_bytes))
    own = ctx is None
    out = Pairwise()
    out.pairs, out.chunks, out.results, out.dd_memory = pairs, chunks, [None] * len(pairs), []
    out.score = np.full((n, n), np.nan, np.float32)
    out.iterations = np.full((n, n), -1, np.int64)
    secs = dict(phase1=0.0, transforms=0.0, nodes=0.0, final=0.0)
    t_start = time.perf_counter()
    src = capi.Context(0 if own else ctx.device_index)
    try:
        if own:
            ctx = capi.Context(0)
        # phase 1 once: the folding beside the all-pairs posteriors (as _phase1_local), no transform
        src.set_sequences(seqs)
        src.fold_begin(0.01)
        try:
            src.align_posteriors(o["align_model"], o["th_a"], fetch=False)
        finally:
            src.fold_end()
        out.sim = src.sim()
        secs["phase1"] = time.perf_counter() - t_start
        for chunk in chunks:
            t = [time.perf_counter()]
            cp = [pairs[k] for k in chunk]
            ctx.pairs_from(src, [x for x, _ in cp], [y for _, y in cp])
            if o["w_pct_f"] != 0.0:
                ctx.fourway_consistency(o["w_pct_f"])
            sims = ctx.sim_blocks()
            ctx.consistency_match(o["w_pct_a"])
            ctx.consistency_bp(o["w_pct_s"])
            t += [time.perf_counter()] * 3  # _phase2_forest's timestamps: fold_launch, pair, pct_fold_tree
            fams = [dict(names=[names[x], names[y]], seqs=[seqs[x], seqs[y]], first=2 * j, sim=sims[j], tree=capi.build_tree(sims[j]))
                    for j, (x, y) in enumerate(cp)]
            res = _phase2_forest(ctx, False, fams, t, o["w"], o["eta0"], o["t_max"], o["th_a"], o["th_s"], o["th_s1"], o["force_iters"],
                                 o["level_sync"], o["slice_iters"], o["skip_uncoupled_folds"], o["round_us"], o["bp_update"],
                                 o["bp_update1"], o["reliability"], False, o["row_structures"])
            secs["transforms"] += t[3] - t[0]
            secs["nodes"] += t[4] - t[3]
            secs["final"] += t[5] - t[4]
            out.dd_memory.append(getattr(res[0], "dd_memory", None))
            for k, (x, y), r in zip(chunk, cp, res):
                it, _, _, sc = r.dd_log[2]
                out.score[x, y] = out.score[y, x] = sc
                out.iterations[x, y] = out.iterations[y, x] = it
                out.results[k] = r
    finally:
        src.close()
        if own and ctx is not None:
            ctx.close()
    secs["total"] = time.perf_counter() - t_start
    out.seconds = secs
    return out


# ------------------------------------------------------------------------------------- each new sequence against a seed
def seed_each_bytes(seed_lens, columns, new_len):
    """Device memory of one new sequence of add_each (bytes; dafs_host_seed_each_bytes): family_bytes of the seed's lengths and
    its own, plus node_bytes(new_len, columns) for its one node against the seed's columns."""
    lens = np.ascontiguousarray([int(x) for x in seed_lens], np.uint32)
    return int(capi._seed_each_bytes(len(lens), lens.ctypes.data, int(columns), int(new_len)))


def seed_scores_tsv(names, each):
    """The table of `dafs --seed SEED --seed-each --seed-scores OUT` (dafs_host_seed_table) for the result of add_each on the
    new sequences `names`: per sequence "j<TAB>name<TAB>length<TAB>matched<TAB>inserted<TAB>score<TAB>iterations" with 1-based j,
    the Stockholm name (stockholm.names over the new sequences' headers) and the floats as %.9g.  A result of add_each with
    seed_ss has four more columns, "pairs<TAB>canonical<TAB>half<TAB>expected" of the sequence's structure support.  A result
    of add_each with nearest has two more at the end (dafs_host_seed_table_nearest): the Stockholm name of the nearest seed row
    ("-" for none) and the identity to it as %.9g."""
    names = list(names)
    if len(names) != len(each.results):
        raise ValueError("seed_scores_tsv: one name per new sequence")
    arrs = [np.ascontiguousarray(a, t) for a, t in ((each.lengths, np.uint32), (each.matched, np.uint32), (each.score, np.float64),
                                                    (each.iterations, np.int64))]
    sup = getattr(each, "support", None)
    near = getattr(each, "nearest", None)
    if sup is None and near is None:
        return capi.host_text(capi._seed_table, len(names), capi.c_strings(names), *[a.ctypes.data for a in arrs])
    if sup is not None:
        arrs += [np.ascontiguousarray(sup[key], t) for key, t in (("both", np.uint32), ("canonical", np.uint32), ("half", np.uint32),
                                                                 ("expected", np.float64))]
    if near is None:
        return capi.host_text(capi._seed_table_support, len(names), capi.c_strings(names), *[a.ctypes.data for a in arrs])
    ptrs = [a.ctypes.data for a in arrs] + [None] * (8 - len(arrs))
    pid = np.ascontiguousarray(near.pid, np.float64)
    return capi.host_text(capi._seed_table_nearest, len(names), capi.c_strings(names), *ptrs,
                          capi.c_strings(["-" if r == NONE else near.names[int(r)] for r in near.row]), pid.ctypes.data)


class AddEach:
    pass


class Merged:
    pass


class Nearest:
    pass


def _merge_each(seed_names, seed_rows, seed_ss, names, seqs, zs, pps, seed_level=None):
    """The merged alignment of add_each from the k column maps zs and the k rows' residue values pps.
    seed_level: the levels of seed_ss -> .ss_level, and .ss_str with each level's bracket kind"""
    m, k, columns = len(seed_rows), len(seqs), len(seed_rows[0])
    seed_col, res_col, width = capi.merge_added(columns, zs)
    mg = Merged()
    mg.z, mg.pp = zs, pps
    mg.names = stockholm.names(seed_names + names)
    cells = np.full((m + k, width), ord("-"), np.uint8)
    cells[:m, seed_col] = np.frombuffer("".join(seed_rows).encode("latin-1"), np.uint8).reshape(m, columns)
    for j in range(k):
        cells[m + j, res_col[j]] = np.frombuffer(seqs[j].encode("latin-1"), np.uint8)
    mg.rows = [row.tobytes().decode("latin-1") for row in cells]
    mg.rf = np.zeros(width, bool)
    mg.rf[seed_col] = True
    if seed_level is None:
        mg.ss = carry_structure(seed_ss, seed_col, width)
        mg.ss_str = capi.make_brackets(mg.ss)
    else:
        mg.ss, mg.ss_level = carry_structure(seed_ss, seed_col, width, seed_level)
        mg.ss_str = capi.make_brackets_levels(mg.ss, mg.ss_level)
    mg.stockholm, mg.col = stockholm.block_merged(mg.names, mg.rows, [None] * m + pps, mg.ss_str, mg.rf)
    lines = [">SS_cons", mg.ss_str]
    for nm, row in zip(seed_names + names, mg.rows):
        lines += ["> " + nm, row]
    mg.output = "\n".join(lines) + "\n"
    return mg


def _select_nr(ctx, mg, m, score, matched, t):
    """The non-redundant subset of a merged alignment (add_each's nr) into mg: .kept, .by, .nr_rows, .nr_names, .nr_stockholm"""
    total = len(mg.rows)
    inc = np.array([r for r in range(total) if r < m or matched[r - m]], np.uint32)  # the rows with a residue in a seed column
    red = ctx.alignment_identity([mg.rows[r] for r in inc], use=mg.rf, nr=t, nearest=False).red
    pos = {int(r): q for q, r in enumerate(inc)}
    order = list(range(m)) + [m + int(j) for j in np.argsort(-np.asarray(score, np.float64), kind="stable")]
    rank = np.array([pos[r] for r in order if r in pos], np.uint32)
    kept, by = capi.nr_select(red, rank, np.arange(len(inc)) < m)
    mg.kept = np.ones(total, bool)
    mg.by = np.full(total, NONE, np.uint32)
    mg.kept[inc] = kept
    mg.by[inc] = np.where(by == NONE, NONE, inc[np.minimum(by, len(inc) - 1)])
    mg.nr_rows = [row for row, keep in zip(mg.rows, mg.kept) if keep]
    mg.nr_names = [nm for nm, keep in zip(mg.names, mg.kept) if keep]
    kept8 = np.ascontiguousarray(mg.kept, np.uint8)
    mg.nr_stockholm = capi.host_text(capi._stockholm_nr, mg.stockholm.encode("latin-1"), total, capi.c_strings(mg.names), kept8.ctypes.data, m, t)


def add_each(seed_names, seed_rows, names, seqs, ctx=None, max_bytes=None, merged=False, nearest=False, nr=None, compare=None, **opts):
    """Each new sequence added to a fixed seed alignment on its own (`dafs --seed SEED --seed-each`).
    opts: the options of add().  results[j] is, bit for bit, what add(seed_names, seed_rows, [names[j]], [seqs[j]], **opts)
    returns (.output, .rows, .ss, .ss_str, .z, .rf, .dd_log and, when asked, .reliability / .stockholm / .row_ss* /
    .covariation), so neither the order of the new sequences nor which others are present matters.

    Phase 1 runs once, in a source context of its own over the m seed sequences and then the k new ones: the folds and the pair
    posteriors of the pairs with a seed sequence on the left (a prefix of the pair ids; no new-new pair), no transform.  The new
    sequences go in chunks, in input order, of at most max_bytes of estimated device memory (seed_each_bytes; default
    DEFAULT_BATCH_BYTES) through `ctx`: Context.families_from builds the chunk's families seed + [new] on the device, then
    the transforms -- the matching transform only for the pairs (seed, new) the node reads
    (Context.consistency_match_pairs), unless reliability asks for the seed-seed rows too -- one node per family, all in
    shared rounds, the merges, and the structures of the whole chunk in one Context.consensus_structures call.  Returns an
    object with .results (one Result per new sequence, in input order), .score and .iterations (the node's final objective
    and iteration count, dd_log's 4th and 1st entries), .lengths, .matched (residues that landed in seed columns), .chunks
    (indices per chunk), .dd_memory (per chunk the nodes' (reserved, in use, peak) bytes) and .seconds (phase1, gather,
    transforms, nodes, final, total; with merged, merge).

    seed_ss, seed_level: as in add().  The seed rows are folded under their constraints once, in the source context; every result's
    structure is the seed's carried into its merged columns, and its .support comes from one Context.structure_support call
    per chunk.  The object gains .support: per new sequence both, canonical, half and expected of its own row.

    merged (`dafs --seed-merged`; needs seed_ss): the object gains .merged, all k placements in one
    alignment, beside the unchanged results.  Columns: capi.merge_added over the k maps, after the last chunk.  .names
    (stockholm.names over the seed's and the new names), .rows (the m seed rows, then the k new rows in input order), .rf,
    .ss / .ss_str (the seed's structure carried into the merged columns), .z (the k maps), .pp (per new row the residue
    values of that row in its own family seed + [j]: one Context.alignment_reliabilities call per chunk that wants the new row
    of every family, so the matching transform stays the listed one), .col (per column the mean of the new rows' values, NaN
    where none has a residue), .stockholm (stockholm.block_merged) and .output (as add prints).

    nearest (`dafs --seed-nearest`): the object gains .nearest with .row, .ident, .den and .pid: for every
    new sequence the seed row nearest to it in the columns of its own result j -- one Context.alignment_identity call per
    result over its printed rows with use = its rf and the seed rows as candidates -- and .names, the seed rows' Stockholm
    names.  A new sequence without a residue in a seed column has no nearest row (NONE, NaN).  The results do not change.

    nr (a threshold in (0, 1]; needs merged; `dafs --seed-nr`): the non-redundant subset of the merged rows.  One
    Context.alignment_identity call over .merged.rows with use = .merged.rf gives the redundancy bits, capi.nr_select the
    subset: the seed rows are forced and visited first, in seed order, then the new rows by descending .score, ties in input
    order.  .merged gains .kept, .by (capi.nr_select), .nr_rows, .nr_names and .nr_stockholm: the merged block without the
    dropped rows and with a `#=GF CC nr T kept K of M hits` line, nothing else changed (dafs_host_stockholm_nr).  A new row
    without a residue in a seed column is compared with nothing and kept.

    compare (run's; it needs merged): .merged.compare, the merged alignment against the reference with use_test = .merged.rf
    -- insert columns are left-justified, not aligned -- and the PP classes of the merged block's own reliabilities."""
    import time
    if compare is not None and not merged:
        raise ValueError(capi.compare_refusal(capi.CMP_NEEDS_MERGED))
    if nr is not None and not merged:
        raise ValueError(capi.alistat_refusal(capi.NR_NEEDS_MERGED))
    if nr is not None and not (0.0 < float(nr) <= 1.0):
        raise ValueError(capi.alistat_refusal(capi.NR_THRESHOLD))
    o = {k: p.default for k, p in inspect.signature(add).parameters.items() if k not in ("seed_names", "seed_rows", "names", "seqs", "ctx")}
    unknown = set(opts) - set(o)
    if unknown:
        raise TypeError("pipeline.add_each: unknown options %s" % sorted(unknown))
    o.update(opts)
    o["th_s1"] = decoder_option(o["decoder"], o["th_s"], o["th_s1"], o["bp_update1"], o["seed_ss"], "pipeline.add_each")
    if o["phylogeny"]:
        raise ValueError(capi.phylogeny_refusal(capi.PHY_NO_SEED_EACH))
    if o.get("phylogeny_bootstrap"):
        raise ValueError(capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE))
    if o.get("phylogeny_transfer"):
        raise ValueError(capi.transfer_refusal(capi.TRANSFER_NEEDS_REPLICATES))
    covariation = cov_options(o["covariation"])
    seed_names, seed_rows = stockholm.clean_seed(seed_names, seed_rows)
    names, seqs = list(names), list(seqs)
    if not seqs or len(names) != len(seqs):
        raise ValueError("pipeline.add_each: at least one new sequence and one name per sequence")
    if any(len(sq) == 0 for sq in seqs):
        raise ValueError("pipeline.add_each: a new sequence has no residues")
    budget = DEFAULT_BATCH_BYTES if max_bytes is None else int(max_bytes)
    if budget < 0:
        raise ValueError("pipeline.add_each: max_bytes is negative")
    m, k = len(seed_rows), len(seqs)
    n = m + 1  # sequences of a family: the seed's, then the new one
    seed_seqs = [r.replace("-", "") for r in seed_rows]
    seed_mask = np.array([[ch != "-" for ch in r] for r in seed_rows], np.uint8)
    columns = seed_mask.shape[1]
    seed_lens = [len(sq) for sq in seed_seqs]
    seed_ss, seed_level, constraints = None, None, None
    if merged and o["seed_ss"] is None:
        raise ValueError(capi._merged_refusal().decode())
    if o["seed_level"] is not None and o["seed_ss"] is None:
        raise ValueError("pipeline.add_each: seed_level gives the levels of seed_ss and needs it")
    if o["seed_ss"] is not None:
        seed_ss, seed_level, constraints = _seed_structure(o["seed_ss"], seed_mask, seed_seqs, o["th_s1"], o["bp_update1"], "pipeline.add_each",
                                                           o["seed_level"])
        constraints += [None] * k
    chunks = pack_families([seed_each_bytes(seed_lens, columns, len(sq)) for sq in seqs], budget)
    th1 = o["th_s"] if o["th_s1"] is None else o["th_s1"]
    prm = capi.dd_params(w=o["w"], eta0=o["eta0"], th_a=o["th_a"], th_s=o["th_s"], t_max=o["t_max"], force_iters=o["force_iters"],
                         skip_uncoupled_folds=1 if o["skip_uncoupled_folds"] else 0)
    # the pairs (s, new) of a family, the only ones its node reads: local id s n - s (s + 1) / 2 + m - s - 1
    node_pairs = np.array([s * n - s * (s + 1) // 2 + m - s - 1 for s in range(m)], np.uint64)
    listed = not o["reliability"] and o["w_pct_a"] != 0.0  # the reliability annotation reads the seed-seed relaxed rows
    out = AddEach()
    out.chunks, out.results, out.dd_memory = chunks, [None] * k, []
    out.score = np.full(k, np.nan, np.float32)
    out.iterations = np.full(k, -1, np.int64)
    out.lengths = np.array([len(sq) for sq in seqs], np.uint32)
    out.matched = np.zeros(k, np.uint32)
    pps = [None] * k  # merged: per new sequence the residue values of its row
    if nearest:
        out.nearest = Nearest()
        out.nearest.names = stockholm.names(seed_names)
        out.nearest.row = np.full(k, NONE, np.uint32)
        out.nearest.ident, out.nearest.den = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        out.nearest.pid = np.full(k, np.nan, np.float64)
    if seed_ss is not None:
        out.support = dict(both=np.zeros(k, np.uint32), canonical=np.zeros(k, np.uint32), half=np.zeros(k, np.uint32),
                           expected=np.zeros(k, np.float64))
    secs = dict(phase1=0.0, gather=0.0, transforms=0.0, nodes=0.0, final=0.0)
    own = ctx is None
    t_start = time.perf_counter()
    src = capi.Context(0 if own else ctx.device_index)
    try:
        if own:
            ctx = capi.Context(0)
        # phase 1 once: the folding beside the pair posteriors of the pairs (x, y) with x < m, no transform
        src.set_sequences(seed_seqs + seqs)
        src.fold_begin(0.01, constraints=constraints)
        try:
            src.align_posteriors(o["align_model"], o["th_a"], 0, m * (m + k) - m * (m + 1) // 2, fetch=False)
        finally:
            src.fold_end()
        secs["phase1"] = time.perf_counter() - t_start
        for chunk in chunks:
            t = [time.perf_counter()]
            ctx.families_from(src, [list(range(m)) + [m + j] for j in chunk])
            t.append(time.perf_counter())
            if o["w_pct_f"] != 0.0:
                ctx.fourway_consistency(o["w_pct_f"])
            ctx.consistency_bp(o["w_pct_s"])
            if listed:
                ctx.consistency_match_pairs(o["w_pct_a"], np.concatenate([node_pairs + np.uint64(f * (n * m // 2)) for f in range(len(chunk))]))
            else:
                ctx.consistency_match(o["w_pct_a"])
            t.append(time.perf_counter())
            nodes = [(f, (np.array([f * n + m], np.uint32), np.ones((1, len(seqs[j])), np.uint8), np.arange(f * n, f * n + m, dtype=np.uint32),
                          seed_mask)) for f, j in enumerate(chunk)]
            outs = [None] * len(chunk)
            batches = iter([nodes])  # every node is ready in the first round, none later

            def finish(f, res, dims):
                outs[f] = res
            _, _, dd_memory, _ = _solve_nodes(ctx, prm, lambda: next(batches, []), finish, slice_iters=o["slice_iters"], round_us=o["round_us"])
            out.dd_memory.append(dd_memory)
            t.append(time.perf_counter())
            # per family add()'s merge of its one map; rows in the order new sequence, seed rows
            alns, rfs = [], []
            for f, j in enumerate(chunk):
                seed_col, res_col, width = capi.merge_added(columns, [outs[f]["z"]])
                mask = np.zeros((n, width), np.uint8)
                mask[0, res_col[0]] = 1
                mask[1:, seed_col] = seed_mask
                rf = np.zeros(width, bool)
                rf[seed_col] = True
                alns.append((np.concatenate([[f * n + m], np.arange(f * n, f * n + m)]).astype(np.uint32), mask))
                rfs.append(rf)
            if seed_ss is None:
                decoded = _decode(ctx, alns, th1)
            else:  # nothing is decoded: the seed's structure in every family's merged columns (seed columns where rf is set)
                decoded = [(carry_structure(seed_ss, np.flatnonzero(rf).astype(np.uint32), len(rf)), None, None) for rf in rfs]
                if seed_level is not None:  # the levels travel with the seed's columns
                    decoded = [(ss, carry_structure(seed_ss, np.flatnonzero(rf).astype(np.uint32), len(rf), seed_level)[1], None)
                               for (ss, *_), rf in zip(decoded, rfs)]
                support = ctx.structure_support(alns, [ss for ss, _, _ in decoded])
            rows_ss = rows_level = rows_auto = [None] * len(chunk)
            if o["row_structures"]:
                lens = {f * n + i: ln for f, j in enumerate(chunk) for i, ln in enumerate(seed_lens + [len(seqs[j])])}
                rows_ss, rows_level, rows_auto = _row_structures(ctx, [sidx for sidx, _ in alns], lens, th1)
            finals = [_final_structure(ctx, sidx, mask, th1, o["bp_update1"], ss) for (sidx, mask), (ss, *_) in zip(alns, decoded)]
            # the annotation, once every structure is final: all rows of every family, or for the merged alignment alone the new
            # row of every family (the first), which reads the listed pairs only
            rls = [None] * len(chunk)
            if o["reliability"]:
                rls = ctx.alignment_reliabilities(alns, finals)
                new_pp = [rl["residue"][:len(seqs[j])] for rl, j in zip(rls, chunk)]
            elif merged:
                new_first = [np.arange(n) == 0] * len(chunk)
                new_pp = [rl["residue"][:len(seqs[j])] for rl, j in zip(ctx.alignment_reliabilities(alns, finals, want=new_first), chunk)]
            if merged:
                for j, pp in zip(chunk, new_pp):
                    pps[j] = pp.copy()
            for f, j in enumerate(chunk):
                res = Result()
                oj = outs[f]
                res.z = [oj["z"]]
                res.rf = rfs[f]
                res.dd_log = {0: (oj["iterations"], oj["violated"], oj["ncbp"], oj["score"])}
                res.dd_memory = dd_memory
                if seed_ss is not None:
                    res.support = _printed_support(support[f], alns[f][0])
                    for key in out.support:  # the new sequence is the first row of its alignment
                        out.support[key][j] = support[f][key][0]
                _final(ctx, res, seed_names + [names[j]], seed_seqs + [seqs[j]], f * n, alns[f][0], alns[f][1], finals[f], rls[f], None,
                       rfs[f], covariation, rows_ss[f], o["identity"], levels=decoded[f][1:], row_level=rows_level[f], row_auto=rows_auto[f])  # no tree per placement: refused above
                out.results[j] = res
                out.score[j] = oj["score"]
                out.iterations[j] = oj["iterations"]
                out.matched[j] = int((np.asarray(oj["z"]) != NONE).sum())
                if nearest and out.matched[j]:  # printed rows: the m seed rows, then the new one
                    idn = ctx.alignment_identity(res.rows, use=rfs[f], cand=np.arange(n) < m)
                    out.nearest.row[j], out.nearest.ident[j], out.nearest.den[j] = idn.nearest[m], idn.nearest_ident[m], idn.nearest_den[m]
                    out.nearest.pid[j] = idn.pid_nearest[m]
            t.append(time.perf_counter())
            for key, a, b in (("gather", 0, 1), ("transforms", 1, 2), ("nodes", 2, 3), ("final", 3, 4)):
                secs[key] += t[b] - t[a]
        if merged:
            t_merge = time.perf_counter()
            out.merged = _merge_each(seed_names, seed_rows, seed_ss, names, seqs, [r.z[0] for r in out.results], pps, seed_level)
            if nr is not None:
                _select_nr(ctx, out.merged, m, out.score, out.matched, float(nr))
            if compare is not None:
                mg = out.merged
                pp_rows = [None] * m
                for row, rel in zip(mg.rows[m:], pps):
                    chars = iter(() if rel is None else [stockholm.pp_char(p) for p in rel])
                    pp_rows.append(None if rel is None else "".join("." if ch == "-" else next(chars) for ch in row))
                mg.compare = compare_result(ctx, compare, mg.names, mg.rows, None if seed_ss is None else mg.ss, use_test=mg.rf,
                                            pp=None if all(r is None for r in pp_rows) else pp_rows)
            secs["merge"] = time.perf_counter() - t_merge
    finally:
        src.close()
        if own and ctx is not None:
            ctx.close()
    secs["total"] = time.perf_counter() - t_start
    out.seconds = secs
    return out


def fold_each(names, seqs, th=0.2, ctx=None, decoder="Nussinov"):
    """Every sequence folded alone: CONTRAfold posteriors (Context.fold_posteriors, no consistency transform), then the MEA
    structure of every sequence's own base-pairing rows at threshold th, all in one Context.consensus_structures call.
    Returns one Result per sequence with .name, .ss (uint32 per residue, NONE for unpaired), .ss_str and .score.
    decoder "Levels" (as in run(); th may then be a sequence, one threshold per level): also .ss_level, and .score holds the
    per-level scores.  th a capi.AutoThresholds: every sequence chooses its own thresholds; as with
    "Levels", and also .ss_auto, its capi.AutoChoice."""
    th = decoder_option(decoder, 0.2 if isinstance(th, capi.AutoThresholds) else th, th, False, None, "pipeline.fold_each")
    names, seqs = list(names), list(seqs)
    if not seqs or len(names) != len(seqs):
        raise ValueError("pipeline.fold_each: at least one sequence and one name per sequence")
    own = ctx is None
    if own:
        ctx = capi.Context(0)
    try:
        ctx.set_sequences(seqs)
        ctx.fold_posteriors(0.01)
        got = ctx.consensus_structures([(np.array([x], np.uint32), np.ones((1, len(s)), np.uint8)) for x, s in enumerate(seqs)], th)
    finally:
        if own:
            ctx.close()
    out = []
    for nm, one in zip(names, got):
        res = Result()
        if _by_level(th):
            res.score, res.ss, res.ss_level = one[:3]
            res.name, res.ss_str = nm, capi.make_brackets_levels(res.ss, res.ss_level)
            if isinstance(th, capi.AutoThresholds):
                res.ss_auto = one[3]
        else:
            score, ss = one
            res.name, res.ss, res.ss_str, res.score = nm, ss, capi.make_brackets(ss), score
        out.append(res)
    return out


# ------------------------------------------------------------------------------------- a mixed input cut into families
class Clustering:
    pass


def _tree_line(score, left, right, names):
    """tree_string of the whole tree without recursion: the guide tree of a large mixed set can be a chain as deep as the set"""
    text = {}
    for i in range(len(score)):  # a join's children have lower indices
        if left[i] < 0:
            text[i] = names[i]
        else:
            text[i] = "[ %g %s %s ]" % (float(score[i]), text.pop(int(left[i])), text.pop(int(right[i])))
    return text[len(score) - 1]


def cluster(names, seqs, threshold=None, count=None, min_size=1, ctx=None, max_bytes=None, linkage="guide", score="sequence",
            structure_weight=None, **opts):
    """Cluster a mixed set of sequences into families and align each (`dafs --cluster`).  The N x N
    similarity matrix of the pair kernels (Context.similarity: the pairs in ranges under max_bytes, so that the set's
    posteriors are never held at once), the guide tree of the whole set (capi.build_tree) and its cut (capi.cluster_cut):
    threshold keeps a join when its score is >= threshold and every join below it is kept, count undoes the joins made last
    until that many clusters are left.  Exactly one of the two.  Every cluster of at least min_size members then goes through
    run_batch (sub-batches under max_bytes; default DEFAULT_BATCH_BYTES for both), so its Result is, bit for bit, what
    run(names_c, seqs_c, **opts) gives.  opts: the options of run() except mp / bp / shard / compare.  With w_pct_f the
    clustering still reads the raw scores; -f acts inside each cluster's run.  linkage: "guide" cuts the guide tree
    (capi.build_tree, on the host); "single", "complete" and "average" cut that linkage tree instead, joined on the device from
    the similarity block the pass has just left there (Context.linkage_tree).  score: "sequence" clusters
    on the pair kernels' similarity score; "structure" and "mix" on the structural pair score or its mix with the sequence
    score at structure_weight (0 .. 1, None: 0.5; an argument of "mix" alone), for which all sequences are folded first with
    the call a run's phase 1 makes (Context.fold_posteriors(0.01)).  .sim, the tree, the cut and the
    table are then those of the chosen matrix; the runs of the clusters are what they are with any score.

    Returns an object with .score, .seq_sim and .struct_sim (the sequence matrix and the structure matrix; .struct_sim is None
    with score "sequence"), .linkage, .sim, .tree = (score, left, right), .tree_line, .labels (uint32 [N]), .clusters (per cluster the
    indices of its members, ascending; the clusters are numbered by their smallest member), .results (per cluster a Result,
    or None below min_size), .ranges (launches of the similarity pass), .table (the text of --cluster-table) and .seconds
    (similarity, tree, batch, total; with a structural score also fold)."""
    import math
    import time
    capi.score_check(score, structure_weight, who="pipeline.cluster")
    for k in ("mp", "bp", "shard"):
        if k in opts:
            raise ValueError("pipeline.cluster: %s is a single-family option (use run)" % k)
    if opts.get("compare") is not None:
        raise ValueError("pipeline.cluster: the clusters are not known in advance; compare is an option of run")
    if opts.get("level_sync") and opts.get("bp_update"):
        raise ValueError("pipeline.cluster: bp_update needs the resident-node schedule (level_sync=False)")
    known = {k: p.default for k, p in inspect.signature(run).parameters.items() if k not in ("names", "seqs", "ctx", "bp", "mp", "shard")}
    unknown = set(opts) - set(known)
    if unknown:
        raise TypeError("pipeline.cluster: unknown options %s" % sorted(unknown))
    cov_options(opts.get("covariation"))
    phylogeny_option(opts.get("phylogeny"), opts.get("phylogeny_bootstrap", 0), opts.get("phylogeny_seed", 12345),
                     opts.get("phylogeny_transfer", False))
    decoder_option(opts.get("decoder", "Nussinov"), opts.get("th_s", known["th_s"]), opts.get("th_s1"), opts.get("bp_update1"), None,
                   "pipeline.cluster")
    names, seqs = list(names), list(seqs)
    n = len(seqs)
    if n == 0 or len(names) != n or any(len(s) == 0 for s in seqs):
        raise ValueError("pipeline.cluster: at least one sequence, none empty, and one name per sequence")
    if (threshold is None) == (count is None):
        raise ValueError("pipeline.cluster: exactly one of threshold and count")
    if threshold is not None and not math.isfinite(float(threshold)):
        raise ValueError("pipeline.cluster: the threshold must be a finite number")
    if count is not None and (int(count) != count or not 1 <= int(count) <= n):
        raise ValueError("pipeline.cluster: count must be 1 .. %d, the number of sequences" % n)
    if int(min_size) != min_size or int(min_size) < 1:
        raise ValueError("pipeline.cluster: min_size must be a positive integer")
    if max_bytes is not None and int(max_bytes) <= 0:
        raise ValueError("pipeline.cluster: max_bytes must be positive")
    if linkage not in capi.LINKAGES:
        raise ValueError("pipeline.cluster: unknown linkage %r (one of %s)" % (linkage, ", ".join(capi.LINKAGES)))
    align_model, th_a = opts.get("align_model", known["align_model"]), opts.get("th_a", known["th_a"])
    own = ctx is None
    if own:
        ctx = capi.Context(0)
    out = Clustering()
    try:
        t0 = tf = time.perf_counter()
        out.score = score
        if n == 1:  # no pair: the unit matrix, no launch
            out.sim, out.ranges = np.ones((1, 1), np.float32), 0
            out.seq_sim, out.struct_sim = out.sim, None if score == "sequence" else out.sim.copy()
        elif score == "sequence":
            ctx.set_sequences(seqs)
            out.sim, out.ranges = ctx.similarity(align_model, th_a, max_bytes)
            out.seq_sim, out.struct_sim = out.sim, None
        else:
            ctx.set_sequences(seqs)
            ctx.fold_posteriors(0.01)  # what phase 1 of a run folds with
            tf = time.perf_counter()
            out.sim, out.ranges = ctx.similarity(align_model, th_a, max_bytes, score=score,
                                                 structure_weight=0.5 if structure_weight is None else float(structure_weight))
            out.seq_sim, out.struct_sim = ctx.pair_scores()
        t1 = time.perf_counter()
        out.linkage = linkage
        if linkage == "guide":
            out.tree = capi.build_tree(out.sim)
        elif n == 1:  # the one-leaf tree
            out.tree = (np.zeros(1, np.float32), np.full(1, -1, np.int64), np.full(1, -1, np.int64))
        else:
            out.tree = ctx.linkage_tree(linkage)
        out.labels, k = capi.cluster_cut(out.tree, threshold=threshold, count=None if count is None else int(count))
        out.clusters = [[] for _ in range(k)]
        for i, c in enumerate(out.labels):
            out.clusters[int(c)].append(i)
        out.tree_line = _tree_line(out.tree[0], out.tree[1], out.tree[2], names)
        out.table = capi.cluster_table(names, [len(s) for s in seqs], out.labels, out.tree, out.sim)
        t2 = time.perf_counter()
        aligned = [c for c, members in enumerate(out.clusters) if len(members) >= int(min_size)]
        res = run_batch([([names[i] for i in out.clusters[c]], [seqs[i] for i in out.clusters[c]]) for c in aligned], ctx=ctx,
                        max_bytes=max_bytes, **opts) if aligned else []
        out.results = [None] * k
        for c, r in zip(aligned, res):
            out.results[c] = r
        t3 = time.perf_counter()
        out.seconds = dict(similarity=t1 - tf, tree=t2 - t1, batch=t3 - t2, total=t3 - t0)
        if score != "sequence":
            out.seconds["fold"] = tf - t0
    finally:
        if own:
            ctx.close()
    return out
