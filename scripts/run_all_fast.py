#!/usr/bin/env python3
"""Counterpart of the search + orthology + clustering steps of SwiftOrtho's scripts/run_all_fast.py (95-193): duplicate
collapse, all-vs-all search on the GPU, expansion, find_orth, clustering.  Same flags for those steps (-i -s -a -v -c -y -n -A -I),
same files under <fasta>_results/ (.sc, .opc, .xyz, .clsr); the species-tree step of the reference (external tools: famsa, trimal, fasttree) is
outside SURVEY.md section 8 and is not run as such: `-t T` (below) builds the tree from the search's own alignments instead.  The operon step (241-255) runs when `-p foo.operon` names a file: scripts/operon_cluster.py
on the .clsr file and the operon file writes <operon name>.xyz (with `-G T`: the shared-family counts on the GPU), and
`bin/find_cluster.py -i` that file with the wrapper's -A, -I and -G writes <operon name>.clsr.  This wrapper keeps its intermediates --
the reference removes every .xyz at its end --, so both files stay.  Without -p nothing of this happens.
The pan-genome step (204-214) runs on request: `-P T` (default `F`: the files and the output above, nothing more) runs scripts/pan_genome.py on the .clsr file after the clustering step and leaves
<name>.pan and <name>.clsr_xy.txt; with `-G T` its counting and rarefaction run on the GPU.  `-C T` (default `F`; with `-P T`) makes that
command also write the gene-content tree of the genomes, <name>.gc.nwk, and the table of the families every pair of genomes shares,
<name>.gc.tsv (pan_genome.py -t -d; Jaccard distances, or `-m overlap`); `-B` and `-S` give the tree bootstrap support as below, with `-G T` on the GPU.
The species-tree step runs on request as well: `-t T` (default `F`) leaves <name>.aln (the core-gene supermatrix of the reference taxon -r,
FASTA, taxa in slot order), <name>.aln.trim (the columns whose share of gaps is at most `-g`, default 1: the same file) and <name>.nwk
(neighbour joining over the `-m p|poisson|kimura|logdet` distances).  The reference shells out to famsa, trimal and fasttree here; this step aligns
nothing: it joins the families along the alignments the search itself made (swiftortho_amd/phy.py), in one process that searches the
proteome once more with a CIGAR on every row; with `-G T` the matrix and the pair counts are built on the GPU.  `-B n` (default 0: the
bare tree) labels the tree's nodes with their bootstrap support over n replicates of the kept columns, drawn from the seed `-S` (default 1)
-- what the reference gets from `fasttree -boot`; with `-G T` the replicates run on the GPU.  `-K T` labels the nodes with their gene
concordance factors (the share of the core families able to decide a branch whose own tree holds it; `boot/gcf` with `-B`) and writes
the table of them to <name>.gcf.tsv.
The phyletic-profile step has no counterpart in the reference and runs on request: `-L T` (default `F`; it needs nothing but the .clsr file)
runs scripts/phyletic_links.py on it with the wrapper's -l and -u and with `-j` (Jaccard threshold, default 0.8) and `-k` (shared genomes at
least, default 2) and leaves <name>.links.tsv, the pairs of gene families that co-occur across the genomes, and <name>.links.xyz; the
modules of such families, <name>.links.clsr, come from `bin/find_cluster.py -i` that .xyz file with the wrapper's -A, -I and -G, as in the
operon step.  With `-G T` the family pairs are found on the GPU.
The gene-fusion step has no counterpart in the reference either and runs on request: `-F T` (default `F`; it needs nothing but the .sc file)
runs scripts/fusion_links.py on it at that script's defaults (this wrapper's -c and -s mean other things) and leaves <name>.fusion.tsv, the
pairs of proteins that align side by side on one composite protein without being homologous, and <name>.fusion.xyz; the modules of such
proteins, <name>.fusion.clsr, come from `bin/find_cluster.py -i` that .xyz file with the wrapper's -A, -I and -G (no link: an empty file).
With `-G T` the links are found on the GPU.
`-l` and `-u` are read by this step alone: the `-P` step runs scripts/pan_genome.py at that script's own defaults (.05, .95), as it always has, so
with other values the families that take part here are not the rows <name>.pan types Share; at the defaults they are.

Clustering step, as the reference has it (139-193): the gene ids of the .opc file are recoded to decimal numbers by first appearance
(<name>.xyz, three columns), THAT file is clustered, and the numbers are mapped back into <name>.clsr (the .grp file in between is
removed).  The recode matters: find_cluster compares ids as strings (`if x > y: continue`, `sort`), and '5' > '12'.
What is NOT the reference here: for `-A mcl` -- its default -- the reference wrapper runs the external `mcl` PROGRAM on the .xyz file
(`mcl ... --abc -te N -I 1.5`; van Dongen's binary, not part of the reference repository and absent from this image).  This wrapper runs
`bin/find_cluster.py -a mcl` (the reference's own Python implementation of the algorithm, SURVEY.md 8f-2, Markov loop on the GPU) on the
same .xyz instead: the two implement the same algorithm with different pruning schemes, so the .clsr of `-A mcl` is not pinned against
the reference wrapper's.  `-A apc` is handed to find_cluster as `-a apc` (affinity propagation, loop on the GPU; ids without '|', so
every gene counts as a taxon of its own in the preference, as in the reference wrapper); `-A sap` is refused by find_cluster.
Addition: `-G T` (default `F`: the commands above) takes the .sc and the .opc file from ONE process, with the hit records expanded and
turned into relations on the GPU (swiftortho_amd.pipeline.orthology_from_search(collapse=True)): same file names, same bytes; one GPU.
The clustering step is the same either way."""
import os
import subprocess
import sys
from time import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swiftortho_amd import nr  # noqa: E402
from swiftortho_amd.fsearch import parse_flags  # noqa: E402

ARGS = {'-i': '', '-r': '', '-p': '', '-s': '1111111', '-c': '.5', '-y': '50', '-n': 'no', '-l': '.05', '-u': '.95', '-a': '1', '-A': 'mcl',
        '-I': '1.5', '-v': '1000', '-G': 'F', '-P': 'F', '-C': 'F', '-t': 'F', '-g': '1', '-m': 'p', '-B': '0', '-S': '1', '-K': 'F',
        '-L': 'F', '-j': '0.8', '-k': '2', '-F': 'F'}


def main(argv):
    a = parse_flags(argv, ARGS)
    if not (a['-B'].isdigit() and a['-S'].isdigit() and int(a['-B']) < 2 ** 31 and int(a['-S']) < 2 ** 64):
        sys.stderr.write('run_all_fast: -B takes a whole number of replicates from 0 to 2^31 - 1, -S a seed from 0 to 2^64 - 1\n')
        return 2
    if a['-i'] == '':
        print('  python %s -i foo.pep.fsa [-s seed] [-a gpus] [-v hits] [-c cov] [-y identity] [-n no|bsr|bal] [-A mcl|apc] [-I 1.5] [-p foo.operon] [-L T [-l .05] [-u .95] [-j 0.8] [-k 2]] [-F T]' % argv[0])
        raise SystemExit()
    fas, name = a['-i'], a['-i'].split(os.sep)[-1]
    t = time()
    opc = '%s_results/%s.opc' % (fas, name)
    sc = '%s_results/%s.sc' % (fas, name)
    if a['-G'].upper()[:1] == 'T':
        # the same two files from one process: duplicates collapsed, searched once, multiplied back and turned into relations on the GPU
        # (pipeline.orthology_from_search(collapse=True)); the .sc is written for the record, nothing reads it
        from swiftortho_amd import pipeline
        os.makedirs(fas + '_results', exist_ok=True)
        lines, _ = pipeline.orthology_from_search(fas, sc_path=sc, coverage=float(a['-c']), identity=float(a['-y']), norm=a['-n'],
                                                  device_stage='relations', collapse=True, **nr.collapsed_search_kw(a['-s'], a['-v']))
        with open(opc, 'wb') as o:
            if lines:
                o.write(b'\n'.join(lines) + b'\n')
        print('all to all homologous searching and orthomcl algorithm time:', time() - t)
    else:
        sc = nr.search_collapsed(fas, a['-s'], a['-a'], a['-v'])
        print('all to all homologous searching time:', time() - t)
        t = time()
        with open(opc, 'wb') as o:
            subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'find_orth.py'), '-i', sc, '-c', a['-c'], '-y', a['-y'], '-n', a['-n'], '-t', 'y'],
                           stdout=o, check=True)
        print('orthomcl algorithm time:', time() - t)
    t = time()
    # gene ids -> numbers by first appearance (run_all_fast.py:143-160)
    xyz, grp, clsr = ('%s_results/%s.%s' % (fas, name, e) for e in ('xyz', 'grp', 'clsr'))
    id2n = {}
    with open(opc) as f, open(xyz, 'w') as o:
        for line in f:
            typ, qid, sid, sco = line.split('\t')
            for g in (qid, sid):
                if g not in id2n:
                    id2n[g] = len(id2n)
            o.write('%d\t%d\t%s' % (id2n[qid], id2n[sid], sco))
    with open(grp, 'wb') as o:
        subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'find_cluster.py'), '-i', xyz, '-a', a['-A'], '-I', a['-I']], stdout=o, check=True)
    # numbers -> gene ids (180-190)
    n2id = {str(n): g for g, n in id2n.items()}
    with open(grp) as f, open(clsr, 'w') as o:
        for line in f:
            o.write('\t'.join(n2id[k] for k in line[:-1].split('\t')) + '\n')
    os.remove(grp)
    print('use %s to group protein family time:' % a['-A'], time() - t)
    if a['-P'].upper()[:1] == 'T':
        # statistics of the pan-genome (run_all_fast.py:204-214): the report into <name>.pan, the curves into <name>.clsr_xy.txt
        t = time()
        with open('%s_results/%s.pan' % (fas, name), 'wb') as o:
            content = []
            if a['-C'].upper()[:1] == 'T':
                gc = '%s_results/%s.gc' % (fas, name)
                content = ['-t', gc + '.nwk', '-d', gc + '.tsv', '-m', a['-m'] if a['-m'] in ('jaccard', 'overlap') else 'jaccard', '-B', a['-B'], '-S', a['-S']]
            subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'pan_genome.py'), '-i', fas, '-g', clsr, '-G', a['-G']] + content, stdout=o, check=True)
        print('pan-genome analysis time:', time() - t)
    if a['-t'].upper()[:1] == 'T':
        # species tree (run_all_fast.py:216-239, without famsa, trimal and fasttree): one process searches the proteome with a CIGAR on every
        # row and joins the core families of -r along those alignments; <name>.aln, <name>.aln.trim (the columns -g keeps) and <name>.nwk
        t = time()
        from swiftortho_amd import phy, pipeline
        gcf = a['-K'].upper()[:1] == 'T'
        newick, sm, st = pipeline.species_tree_from_search(fas, reference=a['-r'], gap_share=float(a['-g']), model=a['-m'],
                                                           device_stage=a['-G'].upper()[:1] == 'T', boot=int(a['-B']), boot_seed=int(a['-S']),
                                                           **dict(nr.collapsed_search_kw(a['-s'], a['-v']), **({'concordance': True} if gcf else {})))
        aln = '%s_results/%s.aln' % (fas, name)
        with open(aln, 'wb') as o:
            o.write(phy.supermatrix_fasta(sm.taxa, sm.matrix, range(sm.matrix.shape[1])))
        with open(aln + '.trim', 'wb') as o:
            o.write(phy.supermatrix_fasta(sm.taxa, sm.matrix, sm.keep))
        with open('%s_results/%s.nwk' % (fas, name), 'wb') as o:
            o.write(newick + b'\n')
        if gcf:
            with open('%s_results/%s.gcf.tsv' % (fas, name), 'wb') as o:
                o.write(phy.gcf_table(sm.taxa, st['gcf']['splits'], st['gcf']['decisive'], st['gcf']['concordant']))
        print('species tree time:', time() - t)
    if a['-L'].upper()[:1] == 'T':
        # phyletic profiles: the pairs of families that co-occur across the genomes, then their modules by the same clustering as above
        t = time()
        links = '%s_results/%s.links' % (fas, name)
        with open(links + '.tsv', 'wb') as o:
            subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'phyletic_links.py'), '-i', fas, '-g', clsr, '-l', a['-l'], '-u', a['-u'], '-j', a['-j'],
                            '-k', a['-k'], '-x', links + '.xyz', '-G', a['-G']], stdout=o, check=True)
        with open(links + '.clsr', 'wb') as o:
            subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'find_cluster.py'), '-i', links + '.xyz', '-a', a['-A'], '-I', a['-I'], '-G', a['-G']], stdout=o, check=True)
        print('phyletic profile time:', time() - t)
    if a['-F'].upper()[:1] == 'T':
        # gene-fusion links: the pairs of proteins that align side by side on one composite, then their modules by the same clustering as above
        t = time()
        fusion = '%s_results/%s.fusion' % (fas, name)
        with open(fusion + '.tsv', 'wb') as o:
            subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'fusion_links.py'), '-i', sc, '-x', fusion + '.xyz', '-G', a['-G']], stdout=o, check=True)
        with open(fusion + '.clsr', 'wb') as o:
            if os.path.getsize(fusion + '.xyz'):
                subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'find_cluster.py'), '-i', fusion + '.xyz', '-a', a['-A'], '-I', a['-I'], '-G', a['-G']], stdout=o, check=True)
        print('gene fusion time:', time() - t)
    if os.path.isfile(a['-p']):
        # operon clustering (run_all_fast.py:241-255): scored operon pairs from the gene families, then the same clustering as above
        t = time()
        oname = a['-p'].split(os.sep)[-1]
        oxyz, oclsr = ('%s_results/%s.%s' % (fas, oname, e) for e in ('xyz', 'clsr'))
        with open(oxyz, 'wb') as o:
            subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'operon_cluster.py'), '-g', clsr, '-p', a['-p'], '-G', a['-G']], stdout=o, check=True)
        with open(oclsr, 'wb') as o:
            subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'find_cluster.py'), '-i', oxyz, '-a', a['-A'], '-I', a['-I'], '-G', a['-G']], stdout=o, check=True)
        print('operon clustering time:', time() - t)
    return 0


if __name__ == '__main__':
    sys.exit(main(list(sys.argv)))
