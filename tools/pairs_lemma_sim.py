#!/usr/bin/env python3
"""CPU simulation for DESIGN.md section 9: chance flags per random 150-base read of the pairs mode's present test ("two pieces within kb
diagonals") against the consecutive-intact-pieces lemma (piece a on diagonal d, piece b on d - k with |a - b| >= k + 1), 96
barcodes of 24 nt, six 4-base pieces, kb = 4.  Output of 4000 reads: 29.7 -> 10.5 flags per read (2.8 x fewer sweeps)."""
import numpy as np, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from biodemux_jl_amd import synth
rng=np.random.default_rng(7)
bcs=synth.make_barcodes(96,24)
P,PL,KB=6,4,4
enc={c:i for i,c in enumerate("ACGT")}
bc=np.array([[enc[c] for c in b] for b in bcs])          # 96 x 24
pk=np.zeros((96,P),dtype=np.int64)
for t in range(P):
    for k in range(PL): pk[:,t]=pk[:,t]*4+bc[:,4*t+k]
n_reads=4000; L=150
cur=ref=0; cur_sw=ref_sw=0
for r in range(n_reads):
    read=rng.integers(0,4,size=L)
    keys=np.zeros(L-PL+1,dtype=np.int64)
    for k in range(PL): keys=keys*4+read[k:L-PL+1+k]
    # H[t][d] = set of barcodes whose piece t matches at diagonal d (position d+4t)
    D=range(-8, L)   # diagonals
    nd=len(D)
    M=np.zeros((96,P,nd),dtype=bool)
    for t in range(P):
        for di,d in enumerate(D):
            p=d+4*t
            if 0<=p<len(keys): M[:,t,di]=pk[:,t]==keys[p]
    once=M.any(axis=1)                       # 96 x nd
    cnt=M.sum(axis=1)
    twice=cnt>=2
    near=np.zeros_like(once)
    for k in range(1,KB+1): near[:,k:]|=once[:,:-k]
    F_cur=twice|(once&near)
    # refined: exists t1<t2 consecutive... use pairwise condition: pieces a at d, b at d-k (k>=0) with |a-b|>=k+1 (k=0: a!=b)
    F_ref=twice.copy()
    for k in range(1,KB+1):
        for a in range(P):
            for b in range(P):
                if abs(a-b)>=k+1:
                    F_ref[:,k:]|=M[:,a,k:]&M[:,b,:-k]
    cur+=F_cur.sum(); ref+=F_ref.sum()
    # sweeps = runs of flagged diagonals per barcode (merged if adjacent)
    def runs(F): return int((F[:,1:]&~F[:,:-1]).sum()+F[:,0].sum())
    cur_sw+=runs(F_cur); ref_sw+=runs(F_ref)
print("flagged (barcode,diagonal) per read: current %.1f refined %.1f ratio %.2f" % (cur/n_reads, ref/n_reads, cur/ref))
print("runs (sweeps) per read: current %.1f refined %.1f ratio %.2f" % (cur_sw/n_reads, ref_sw/n_reads, cur_sw/ref_sw))
