"""Device-resident problem state for the block-simplex LSQ hot path (MI355X).

HBM layout of one z-space problem (python/main.py:41-79 restated for the GPU):
  A      CSR, m x n: int64 indptr, int32 indices, fp64 data     (SpMV,  K1)
  A'     CSR, n x m: the explicit transpose (no atomics)         (SpMV', K2)
  target m fp64 = A x0 - b (python/main.py:48)
  x      n fp64 = N z (never materialised N: per-block differences; x0 is in target)
  r      m fp64 residual
  z[2], g[2]   ping-pong iterate / gradient buffers, n_z = n - p fp64 each
  xstarts, zstarts  p int64 block starts in x and z; xz n int32 (z index of an
               x entry, -1 for a block's last entry) -- the N' adjacency
  scal   16 fp64 device scalars (t, f, BB sums, stop flag, iteration)
All compute is in lib/libbsls_hip.so; the host layer only owns buffers and
sequences calls.  This module is its public face; the code lives in
  dev_images  the CSR / panel / tile images, their planners and NumPy models
  dev_blocks  the block layout and the isotonic pack plan
  dev_lsq     the x-space operator pair and XBBEngine
  dev_bb      BBEngine, its option checks, the line search, the BB host loop
  dev_batch   BatchBB
  dev_metrics the link metrics of a fit by set and flow class (GEH, RMSE, ..)
Importing it needs neither a GPU nor torch.
"""
from dev_images import (NT_BYTES, DeviceCSR, DevicePanels, DeviceTiles, PanelOverflow,
                        _dealt_matvec, build_panels, chunk_plan, even_bounds, k1_plan,
                        panel_rows, panels_matvec, scaled_incidence_scale, self_bytes,
                        spmv_format, tile_plan, tiles_matvec, value_codec)
from dev_blocks import BlockLayout, IsoPlan, _cur_dev, _iso_plans, iso_mode, iso_plan
from dev_lsq import DeviceLSQ, XBBEngine, lsq_operator
from dev_bb import (BBEngine, LineSearch, fixed_plan_fits, fixed_sum_bounds, fixed_sums_check,
                    reg_lambda_check, reg_model, reg_weights_check, row_weights_check)
from dev_batch import BatchBB, _batch_columns, batch_groups, batch_width
from dev_metrics import KEYS, link_classes, link_metrics, metrics_from_cells
