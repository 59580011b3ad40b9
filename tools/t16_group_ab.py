"""Same-box A/B of tile16's tile grouping (tiny_batch_set_tile_grouping) against its tail stride (tiny_batch_set_tile_queue): kernel ms of a cold-start
launch in predicted longest-first order with tiles in index order (g0) and tiles formed by window start (g1), for several strides and batch sizes,
`passes` passes each (the configurations alternate inside a pass), and a check that the results do not depend on either.  (The cost of building
the map is read from a kernel trace: instance_map_kernel.)
    python tools/t16_group_ab.py [strides] [batches] [passes] [shuffle]"""
import sys, numpy as np
sys.path.insert(0, '.')
import accelerated_tinympc_amd as T
pr = T.problems
prob = pr.quadrotor(20, 30)
strides = [int(s) for s in (sys.argv[1] if len(sys.argv) > 1 else "-1").split(",")]
batches = [int(s) for s in (sys.argv[2] if len(sys.argv) > 2 else "65536").split(",")]
passes = int(sys.argv[3]) if len(sys.argv) > 3 else 2
shuffle = len(sys.argv) > 4 and sys.argv[4] == "shuffle"
for B in batches:
    x0, table, start = pr.tracking_batch(B, 30)
    if shuffle:
        perm = np.random.default_rng(1).permutation(B); x0, start = x0[perm], start[perm]
    sol = T.TinyBatchSolver(prob, B); sol.set_dispatch(1); sol.select_kernel(2); sol.set_row_kernel(5)
    sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start); sol.enable_timing(True)
    ref = None; ms = {}; differ = False
    for p in range(passes):
        for g in (0, 1):
            for k in strides:
                sol.set_tile_grouping(g); sol.set_tile_queue(k)
                for r in range(8):
                    sol.reset_workspace(); sol.set_x0(x0); sol.solve_async(); sol.synchronize()
                    if r >= 2: ms.setdefault((g, k), []).append(sol.last_solve_ms())
                st = dict(zip(("iter", "status", "residuals"), sol.get_status()), u=sol.get_u())   # (the bitwise tests compare every work array)
                if ref is None: ref = st
                differ |= not all(np.array_equal(st[a].view(np.uint32) if st[a].dtype == np.float32 else st[a], ref[a].view(np.uint32) if ref[a].dtype == np.float32 else ref[a]) for a in st)
    line = [f"g{g} stride {k:3d}: {np.median(v):.4f} (min {min(v):.4f})" for (g, k), v in sorted(ms.items())]
    print(f"B={B:7d}{' shuffled' if shuffle else ''} {sol.kernel_name()} mean iters {ref['iter'].mean():.2f} tiles/slot {(B + 15) // 16 / 1024:.2f}{'  RESULTS DIFFER' if differ else ''}\n    " + "\n    ".join(line), flush=True)
    sol.close()
