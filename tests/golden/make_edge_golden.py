#!/usr/bin/env python3
"""Generates tests/golden/edge_golden.npz: what the COMPILED REFERENCE (oracle/_ref/libstage_ref.so, oracle/ref_stage_shim.cpp) makes of the reads at sequence
ends of tests/edge_gen.py -- mem_chain_Learned + mem_chain_flt on the workload's seeds with the ALT flags, then mem_chain2aln_across_reads_V2 (its own
BandedPairWiseSW kernels) on those chains, both under the default options.  Runs in the build container (no GPU).  Data only: the reference's outputs; the
inputs are regenerated from a seed by the tests."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "bwa-meme_amd"))
import edge_gen as EG  # noqa: E402
import oracle_py as O  # noqa: E402
import ref_py  # noqa: E402


def main(out):
    W = EG.workload()
    copt = O.default_chain_opt(W["l_pac"])
    n = W["read_off"].shape[0] - 1
    ch_list, sd_list, frac, tree, coff, soff = [], [], [], [], [0], [0]
    for r in range(n):
        rc, ch, sd, tr, fr = ref_py.chain_read(W["smems"][r, :W["n_smems"][r]], W["hits"][r, :W["n_hits"][r]], int(W["read_off"][r + 1] - W["read_off"][r]),
                                               W["contig_off"], W["contig_len"], W["contig_alt"], copt)
        assert rc >= 0
        ch_list.append(ch); sd_list.append(sd); frac.append(np.float32(fr)); tree.append(tr)
        coff.append(coff[-1] + rc); soff.append(soff[-1] + sd.shape[0])
    chains, seeds = np.concatenate(ch_list), np.concatenate(sd_list)
    chain_off, seed_off = np.array(coff, np.int64), np.array(soff, np.int64)
    frac = np.array(frac, np.float32)
    regs = ref_py.extend_reads(W["reads"], W["read_off"], chain_off, chains, seed_off, seeds, frac, W["text"], W["l_pac"], W["contig_off"], W["contig_len"],
                               W["contig_alt"], O.default_ext_opt())
    np.savez_compressed(out, chain_off=chain_off, chains=np.stack([chains[f].astype(np.int64) for f in EG.CHAIN_FIELDS], 1),
                        seeds=EG.chain_seeds(chain_off, chains, seed_off, seeds), tree_size=np.array(tree, np.int32), frac_rep_bits=frac.view(np.uint32),
                        reg_off=seed_off, regs=np.stack([regs[f].astype(np.int64) for f in O.ALNREG_FIELDS], 1), reg_frac_bits=regs["frac_rep"].view(np.uint32))
    live = regs["qe"] > regs["qb"]
    print("reads", n, "chains", chains.shape[0], "records", regs.shape[0], "live", int(live.sum()), "at the text's ends and the junction",
          [int((live & m).sum()) for m in (regs["rb"] == 0, regs["re"] == 2 * W["l_pac"], regs["re"] == W["l_pac"], regs["rb"] == W["l_pac"])])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "edge_golden.npz"))
