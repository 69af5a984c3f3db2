"""One population + neighbour call at 400 and at 401 columns (kernel trace of the dispatch seam).
Run from the repository root under
`rocprofv3 --kernel-trace --stats -- python scratch/wide_seam.py`."""
import sys
import torch
sys.path.insert(0, ".")
from clustering_amd import density as dens
from clustering_amd.synth import gaussian_blobs
for D in (400, 401):
    ct = torch.from_numpy(gaussian_blobs(4096, D, seed=3)).cuda()
    p = dens.calculate_populations_partial(ct, [1.0])
    fe = dens.calculate_free_energies(p[0].contiguous())
    dens.nearest_neighbors_partial(ct, fe)
torch.cuda.synchronize()
print("seam ok")
