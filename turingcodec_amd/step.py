"""The primitive step of one picture on the device, and the frame-parallel slot loop around it.

DeviceFrame   a FrameWorkload (turingcodec_amd/workload.py: the reference encoder's measured call mix of one picture) uploaded to HBM + the list of batch launches
              that make one step, in independent chains; fork/join lanes, the lane planner, HIP-graph capture, per-group kernel times, checksums.
FramePipeline time slot t of frame_parallel.DagSchedule on one rank: references out of the DPB mirror, the picture's step, padding, staging, the broadcasts.

Moved here from bench.py in round 6: the orchestration of a step is the product's; bench.py only measures it."""
import numpy as np


class DeviceFrame:
    """A FrameWorkload uploaded to HBM + the list of launches that make one step."""

    def __init__(self, hv, wl, use_planes=True, fused_tu=True, ime_range=None, skip=(), rdoq=True, pred_launches="merged", scan_in_forward=True, sad4_runs=True):
        import torch
        self.sad4_runs = sad4_runs
        from turingcodec_amd import havoc as _havoc
        self.rdoq = bool(rdoq) and wl.mix == "ra"
        self.skip = set(skip)   # diagnostic only: launch groups left out of the step (marginal-cost measurements)
        self.hv, self.wl, self.use_planes, self.fused_tu, self.ime_range = hv, wl, use_planes, fused_tu, ime_range
        self.pred_launches, self.scan_in_forward = pred_launches, scan_in_forward
        up = hv.up
        dt = wl.dtype
        S = wl.S
        # picture store: 3 input planes + plane 3 = reconstruction
        store = np.concatenate([wl.luma, np.zeros(wl.plane_len, dt)])
        self.luma = up(store)
        self.chroma = up(np.concatenate([wl.chroma, np.zeros(2 * wl.cplane_len, dt)]))   # + planes 3 / 4: reconstructed Cb / Cr
        z = lambda n, d: hv.zeros(n, d)
        self.pred = z(wl.pred_len, dt)
        self.cpred = z(wl.cpred_len, dt)
        self.bi = z(wl.bi_len + 4096, dt)
        self.cbi = z(len(wl.bi4) * 1024 + 1024, dt)     # chroma bi predictions: own slots (32 x 32, stride 32)
        self.sbi = z(len(wl.subtract_bi) * 4096, dt)
        self.j_sad4, self.j_sad = up(wl.sad4), up(wl.sad)
        # the calls of a search follow each other in the table: the host cutter makes them runs (boxes of their candidates; lengths by block size)
        self.j_runs = up(hv.sad4_make_runs(wl.sad4, 0, wl.stride, wl.S)) if sad4_runs and len(wl.sad4) else None
        self.o_sad4, self.o_sad = z(4 * len(wl.sad4), np.int32), z(len(wl.sad), np.int32)
        if ime_range is not None:   # integer ME from SAD surfaces: one (2R+1)^2 surface per search instead of SAD4 jobs
            side = 2 * ime_range + 1
            sj = np.zeros((len(wl.me_search), 8), np.int32)
            sj[:, :4] = wl.me_search
            sj[:, 4] = np.arange(len(sj)) * side * side
            self.j_surf, self.o_surf = up(sj), z(len(sj) * side * side, np.int32)
        self.j_sbi = up(wl.subtract_bi)
        self.j_satd = up(wl.satd_inter)
        self.o_satd = z(len(wl.satd_inter), np.int32)
        self.subpel = {hi: dict(jobs=up(j), cost=z(len(j), np.int32)) for hi, j in wl.subpel.items() if len(j)}
        if self.use_planes:
            pl = wl.plane_len
            self.planes = z(32 * pl, dt)                       # [ref L0 | ref L1] x 16 phase planes
            self.planes[0:pl].copy_(self.luma[pl:2 * pl])      # slot 0 of each reference = the picture itself
            self.planes[16 * pl:17 * pl].copy_(self.luma[2 * pl:3 * pl])
            self.subpel_planes = {c: dict(jobs=up(j), cost=z(16 * len(j), np.int32)) for c, j in wl.subpel_planes.items() if len(j)}
        self.intra = {}
        for log2, j in wl.intra.items():
            if len(j):
                self.intra[log2] = dict(jobs=up(j), nb=up(wl.intra_nb[log2]), dst=z(len(j) << (2 * log2), dt))
        self.isearch = {}
        for log2, j in wl.intra_search.items():
            if len(j):
                self.isearch[log2] = dict(jobs=up(j), nb=up(wl.intra_search_nb[log2]), cost=z(35 * len(j), np.int32))
        self.tu = {}
        bd = wl.bit_depth
        qp = wl.qp
        from turingcodec_amd.workload import quant_params, dequant_params
        for (log2, tr), g in wl.tu.items():
            m = len(g["jobs"])
            if not m:
                continue
            nn = g["n"]
            # quantiser parameters exactly as turing/QpState.h:85-94 / Reconstruct.cpp:286,311,315 derive them
            qscale, qshift, qoffset = quant_params(qp, log2, bd, wl.mix == "ai")
            dscale, dshift = dequant_params(qp, log2, bd)
            qj = np.zeros((m, 8), np.int32)
            qj[:, 0] = qj[:, 1] = g["jobs"][:, 0]
            qj[:, 2] = nn * nn
            qj[:, 3], qj[:, 4], qj[:, 5] = qscale, qshift, qoffset
            dj = qj.copy()
            dj[:, 3], dj[:, 4] = dscale, dshift
            self.tu[(log2, tr)] = dict(jobs=up(g["jobs"]), src=up(g["src"]), res_off=up(g["res_off"]), n=nn,
                                       res=z(m * nn * nn, np.int16), coef=z(m * nn * nn, np.int16),
                                       level=z(m * nn * nn, np.int16), deq=z(m * nn * nn, np.int16),
                                       qjobs=up(qj), djobs=up(dj), cbf=z(m, np.int32), rec=z(m * nn * nn, dt),
                                       jssd=up(g["ssd"]), ossd=z(len(g["ssd"]), np.uint32), dscale=dscale, dshift=dshift)
            fj = g["jobs"].copy()
            fj[:, 1] = g["src"][:, 0]          # havoc_mi355x_tu_fused_job: coef_off, src_off, pred_off, rec_off
            extra = g["ssd"][m:]
            self.tu[(log2, tr)].update(fjobs=up(fj), jssd_x=up(extra) if len(extra) else None, ossd_x=z(max(1, len(extra)), np.uint32))
            if self.rdoq:
                rj = wl.rdoq_jobs((log2, tr), _havoc.rdoq_lambda(wl.rdoq_lambda, dscale))
                self.tu[(log2, tr)]["rjobs"] = torch.from_numpy(rj.view(np.uint8).reshape(-1)).to(hv.device)
                self.tu[(log2, tr)]["rwork"] = hv.rdoq_workspace(len(rj))
        self.rdoq_states = torch.from_numpy(np.ascontiguousarray(wl.rdoq_states).reshape(-1)).to(hv.device)
        # final reconstruction pass of the picture (workload.recon): what later pictures predict from
        self.recon = {}
        for comp, tabs in wl.recon.items():
            for log2, g in tabs.items():
                dscale, dshift = dequant_params(qp, log2, bd)
                self.recon[(comp, log2)] = dict(jobs=up(g["jobs"]), levels=up(g["levels"]), ssd=z(len(g["jobs"]), np.uint32), n=g["n"],
                                                dscale=dscale, dshift=dshift)
        self.dbk_data = torch.from_numpy(np.ascontiguousarray(wl.deblock_blocks[0])).to(hv.device)
        self.dbk_bs = torch.from_numpy(np.ascontiguousarray(wl.deblock_blocks[1])).to(hv.device)
        # pristine copy of the synthetic reference planes: what a picture WITHOUT references (the IDR of the frame-parallel
        # schedule) predicts from, whatever an earlier picture left in the store
        self.init_refs = (self.luma[wl.plane_len:3 * wl.plane_len].clone(), self.chroma[wl.cplane_len:3 * wl.cplane_len].clone())
        self.launches = self._make_launches()
        torch.cuda.synchronize()   # every upload / fill above has landed, whatever stream it ran on, before the first launch
        # --rdoq 0 (round 1's step): levels for the timed de-quantiser from residual -> forward T -> havoc_quantize once,
        # untimed.  Default: Rdoq::runQuantisation is in the timed chain (havoc_quantize in the all-intra speed=fast mix).
        if not self.rdoq:
            for name, fn in self.launches:
                if name.startswith(("residual", "transform", "tu_forward")):
                    fn()
            for g in self.tu.values():
                hv.quantize_d(g["level"], g["coef"], g["qjobs"], g["cbf"])
        hv.sync()

    def _make_launches(self):
        hv, wl = self.hv, self.wl
        bd, st, cst = wl.bit_depth, wl.stride, wl.cstride
        L = []
        chains = []   # lists of indices into L: launches of one chain depend on each other, chains are independent

        def chain(*items):
            items = [it for it in items if it[0] not in self.skip]
            if items:
                chains.append(list(range(len(L), len(L) + len(items))))
                L.extend(items)

        inter = wl.mix == "ra"
        if not inter:
            pass
        elif self.ime_range is None:
            if self.j_runs is not None:
                chain(("sad4", lambda: hv.sad4_runs_d(self.luma, st, self.luma, st, self.j_sad4, self.j_runs, self.o_sad4)))
            else:
                chain(("sad4", lambda: hv.sad4_d(self.luma, st, self.luma, st, self.j_sad4, self.o_sad4)))
        else:
            chain(("sad_surface", lambda: hv.sad_surface_d(self.luma, st, self.luma, st, self.ime_range, 64, 64, self.j_surf, self.o_surf)))
        if inter:
            chain(("sad", lambda: hv.sad_d(self.luma, st, self.luma, st, self.j_sad, self.o_sad)))
        if not inter:
            pass
        elif self.use_planes:
            # sub-pel candidates against phase planes: interpolate each reference picture once (streaming, HBM-bound),
            # then every group of 16 candidates is one SATD job between the source PU and 16 blocks of the right planes
            pl, m = wl.plane_len, wl.plane_margin
            x0, y0, rw, rh = 96 - m, 96 - m, wl.width + 2 * m, wl.height + 2 * m
            items = [("interp_planes", lambda r=r: hv.interp_planes_d(bd, self.planes[16 * r * pl:], pl, self.luma[(1 + r) * pl:], st, x0, y0, rw, rh))
                     for r in (0, 1)]
            for (mw, mh), g in sorted(self.subpel_planes.items(), reverse=True):
                items.append(("satd_planes", lambda g=g, mw=mw, mh=mh: hv.satd_multi_d(self.luma, st, self.planes, st, g["jobs"], g["cost"], mw, mh)))
            chain(*items)
        else:
            for hi, g in sorted(self.subpel.items(), reverse=True):
                chain(("subpel_satd", lambda g=g, hi=hi: hv.subpel_satd_d(8, bd, hi, hi, self.luma, st, self.luma, st, g["jobs"], g["cost"])))
        def classes(name, jobs, wcol, fn):
            """one launch per block-size class (the reference's table is indexed by width class)"""
            jobs_np = np.asarray(jobs)
            return [(name, lambda j=hv.up(np.ascontiguousarray(jobs_np[idx])), mw=mw, mh=mh: fn(j, mw, mh))
                    for idx, mw, mh in hv.size_classes(jobs_np[:, wcol], jobs_np[:, wcol + 1])]

        if inter and self.pred_launches == "merged":
            # all four size classes of a table in ONE launch (havoc_mi355x_pred_*_classes): 4 prediction launches per picture instead of 16
            def merged(name, jobs, wcol, bi, taps, dst, sd, ref, sr):
                srt, counts, _ = hv.sort_by_class(np.asarray(jobs), np.asarray(jobs)[:, wcol], np.asarray(jobs)[:, wcol + 1])
                return (name, lambda j=hv.up(srt), c=counts: hv.pred_classes_d(bi, taps, bd, dst, sd, ref, sr, j, c))
            chain(merged("pred_uni8", wl.uni8, 2, False, 8, self.pred, 64, self.luma, st),
                  ("satd_inter", lambda: hv.satd_d(self.luma, st, self.pred, 64, self.j_satd, self.o_satd)))
            chain(merged("pred_uni4", wl.uni4, 2, False, 4, self.cpred, 32, self.chroma, cst))
            chain(merged("pred_bi8", wl.bi8, 3, True, 8, self.bi, 64, self.luma, st),
                  ("subtract_bi", lambda: hv.subtract_bi_d(bd, self.sbi, 64, self.bi, 64, self.luma, st, self.j_sbi)),
                  merged("pred_bi4", wl.bi4, 3, True, 4, self.cbi, 32, self.chroma, cst))
        elif inter:
            chain(*classes("pred_uni8", wl.uni8, 2, lambda j, mw, mh: hv.pred_uni_d(8, bd, self.pred, 64, self.luma, st, j, mw, mh)),
                  ("satd_inter", lambda: hv.satd_d(self.luma, st, self.pred, 64, self.j_satd, self.o_satd)))
            chain(*classes("pred_uni4", wl.uni4, 2, lambda j, mw, mh: hv.pred_uni_d(4, bd, self.cpred, 32, self.chroma, cst, j, mw, mh)))
            chain(*classes("pred_bi8", wl.bi8, 3, lambda j, mw, mh: hv.pred_bi_d(8, bd, self.bi, 64, self.luma, st, j, mw, mh)),
                  ("subtract_bi", lambda: hv.subtract_bi_d(bd, self.sbi, 64, self.bi, 64, self.luma, st, self.j_sbi)),
                  *classes("pred_bi4", wl.bi4, 3, lambda j, mw, mh: hv.pred_bi_d(4, bd, self.cbi, 32, self.chroma, cst, j, mw, mh)))
        for log2, g in sorted(self.isearch.items(), reverse=True):
            chain(("intra_satd35", lambda g=g, log2=log2: hv.intra_satd35_d(bd, log2, self.luma, st, g["nb"], g["jobs"], g["cost"])))
        for log2, g in sorted(self.intra.items(), reverse=True):
            n = 1 << log2
            chain(("intra", lambda g=g, log2=log2, n=n: hv.intra_d(bd, log2, g["dst"], n, g["nb"], g["jobs"])))
        for (log2, tr), g in sorted(self.tu.items(), reverse=True):
            n = g["n"]
            # speed=medium: tu_forward -> Rdoq::runQuantisation -> tu_reconstruct, one dependent chain on the device.  With
            # --rdoq 0 the two halves are independent (levels pre-computed, untimed, in __init__)
            rdq = ("rdoq", lambda g=g, log2=log2: hv.rdoq_d(bd, log2, g["level"], g["coef"], self.rdoq_states, g["rjobs"], g["cbf"], g["rwork"]))
            if self.fused_tu:
                # residual + forward transform in one kernel; de-quant + inverse transform + add + SSD in another
                fwd = ("tu_forward", lambda g=g, log2=log2, tr=tr: hv.tu_forward_d(bd, tr, log2, g["coef"], self.luma, st, self.luma, st, g["fjobs"]))
                items = [("tu_reconstruct", lambda g=g, log2=log2, tr=tr, n=n: hv.tu_reconstruct_d(
                    bd, tr, log2, g["dscale"], g["dshift"], g["rec"], n, self.luma, st, self.luma, st, g["level"], g["fjobs"], g["ossd"]))]
                if g["jssd_x"] is not None:   # the reference makes ~1.26 SSD calls per TU: the rest as plain SSD jobs
                    items.append(("ssd", lambda g=g, n=n: hv.ssd_d(self.luma, st, g["rec"], n, g["jssd_x"], g["ossd_x"])))
                if self.rdoq and self.scan_in_forward and log2 >= 4 and tr == 0:
                    # 16x16 / 32x32: the scan pass of the device RDOQ runs inside tu_forward (the coefficients are in registers there)
                    chain(("tu_forward", lambda g=g, log2=log2: hv.tu_forward_scan_d(bd, log2, g["coef"], self.luma, st, self.luma, st, g["fjobs"], g["rjobs"],
                                                                                      g["level"], g["rwork"])),
                          ("rdoq", lambda g=g, log2=log2: hv.rdoq_prescanned_d(bd, log2, g["level"], g["coef"], self.rdoq_states, g["rjobs"], g["cbf"], g["rwork"])),
                          *items)
                elif self.rdoq:
                    chain(fwd, rdq, *items)
                elif inter:
                    chain(fwd)
                    chain(*items)
                else:   # speed=fast: no RDOQ -- havoc_quantize sits between the two halves, one dependent chain on the device
                    chain(fwd, ("quantize", lambda g=g: hv.quantize_d(g["level"], g["coef"], g["qjobs"], g["cbf"])), *items)
                continue
            front = [("residual", lambda g=g, n=n: hv.residual_d(g["res"], n, g["res_off"], self.luma, st, self.luma, st, g["src"])),
                     ("transform", lambda g=g, n=n, log2=log2, tr=tr: hv.transform_d(bd, tr, log2, g["coef"], g["res"], n, g["jobs"]))]
            back = [("quantize_inverse", lambda g=g: hv.quantize_inverse_d(g["deq"], g["level"], g["djobs"])),
                    ("inverse_transform_add", lambda g=g, log2=log2, tr=tr, n=n: hv.inverse_transform_add_d(
                        bd, tr, log2, g["rec"], n, self.luma, st, g["deq"], g["jobs"])),
                    ("ssd", lambda g=g, n=n: hv.ssd_d(self.luma, st, g["rec"], n, g["jssd"], g["ossd"]))]
            if self.rdoq:
                chain(*front, rdq, *back)
            else:
                chain(*front)
                chain(*back)
        if inter and "recon" not in self.skip:
            # the chosen modes' reconstruction of the whole picture, every sample once, into the reconstruction planes
            items = []
            for (comp, log2), g in sorted(self.recon.items(), key=lambda kv: (-kv[0][1], kv[0][0])):
                plane, stv = (self.luma, st) if comp == "y" else (self.chroma, cst)
                items.append(("recon", lambda g=g, log2=log2, plane=plane, stv=stv: hv.tu_reconstruct_d(
                    bd, 0, log2, g["dscale"], g["dshift"], plane, stv, plane, stv, plane, stv, g["levels"], g["jobs"], g["ssd"])))
            # then the in-loop deblocking filter over the whole picture (turing/TaskDeblock.cpp:105-127): what a reference
            # picture looks like when later pictures predict from it
            pl_, cpl_ = wl.plane_len, wl.cplane_len
            if "deblock" not in self.skip:
                items.append(("deblock", lambda: hv.deblock_d(bd, self.luma, 3 * pl_ + 96 * st + 96, st, self.chroma, 3 * cpl_ + 48 * cst + 48,
                                                               4 * cpl_ + 48 * cst + 48, cst, wl.width, wl.height, self.dbk_data, self.dbk_bs)))
            chain(*items)
        self.chains = chains
        return L

    def step(self, nlanes=1):
        """issue one frame's launches; with nlanes > 1 the independent chains go onto fork/join lanes: round-robin, or as
        `self.assign` (list of chain-index lists, one per lane; see plan_lanes) says"""
        if nlanes <= 1:
            for _, fn in self.launches:
                fn()
            return
        hv = self.hv
        assign = getattr(self, "assign", None) or [list(range(k, len(self.chains), nlanes)) for k in range(nlanes)]
        hv.fork(nlanes)
        for k, lane in enumerate(assign):
            hv.lane(k)
            for ci in lane:
                for idx in self.chains[ci]:
                    self.launches[idx][1]()
        hv.join()

    def chain_times_ms(self):
        """isolated duration of every chain (sum of its launches), for the lane planner"""
        hv, out = self.hv, []
        for ch in self.chains:
            run = lambda: [self.launches[i][1]() for i in ch]
            run()
            hv.timer_start()
            for _ in range(3):
                run()
            out.append(hv.timer_stop_ms() / 3)
        return out

    def plan_lanes(self, nlanes, ntry, seed=1):
        """Host-side scheduling of the step: which independent chain goes to which lane, in which order.  Candidates:
        round-robin, longest-chain-first onto the least loaded lane (LPT), seeded perturbations of LPT, then a local
        search (single-chain moves) around the best; each candidate is captured into a HIP graph and timed, the fastest is
        kept (returns the graph).  Set-up work, outside any timed region -- like planning an FFT."""
        import random
        hv = self.hv
        cost = self.chain_times_ms()
        rnd = random.Random(seed)

        def lpt(noise):
            order = sorted(range(len(cost)), key=lambda c: -cost[c] * (1.0 + noise * rnd.uniform(-1, 1)))
            lanes, load = [[] for _ in range(nlanes)], [0.0] * nlanes
            for c in order:
                k = load.index(min(load))
                lanes[k].append(c)
                load[k] += cost[c]
            return lanes

        def measure(cand):
            self.assign = cand
            g = hv.graph_capture(lambda: self.step(nlanes))
            for _ in range(2):
                hv.graph_launch(g)
            hv.sync()
            ms = 1e30
            for _ in range(3):   # best of three batches: one noisy batch must not decide the plan
                hv.timer_start()
                for _ in range(8):
                    hv.graph_launch(g)
                ms = min(ms, hv.timer_stop_ms() / 8)
            return g, ms

        best = (None, None, 1e30)
        self._planned_graphs = getattr(self, "_planned_graphs", [])

        def offer(cand):
            nonlocal best
            g, ms = measure(cand)
            self._planned_graphs.append(g)   # losers are kept until the process ends: destroying executable graphs right
            if ms < best[2]:                 # after use crashed the runtime intermittently (3 of 8 runs, ROCm 7.0)
                best = (cand, g, ms)
                return True
            return False

        # a third of the budget on constructive candidates, the rest on a local search around the best one: move one chain
        # to another lane / position, keep the move when the measured step gets faster
        first = max(1, min(ntry, 2 + ntry // 3))
        cands = [None, lpt(0.0)] + [lpt(0.5) for _ in range(max(0, first - 2))]
        for cand in cands[:first]:
            offer(cand)
        for _ in range(max(0, ntry - first)):
            cur = best[0] if best[0] is not None else [list(range(k, len(self.chains), nlanes)) for k in range(nlanes)]
            cand = [list(l) for l in cur]
            src = rnd.choice([k for k in range(nlanes) if cand[k]])
            c = cand[src].pop(rnd.randrange(len(cand[src])))
            dst = rnd.randrange(nlanes)
            cand[dst].insert(rnd.randint(0, len(cand[dst])), c)
            offer(cand)
        self.assign = best[0]
        return best[1], best[2]

    def kernel_times_ms(self, reps):
        """average duration per launch group, HIP events on the context's stream"""
        hv = self.hv
        t = {}
        cnt = {}
        for name, fn in self.launches:
            fn()
            ms = None
            for _ in range(3):   # best of three averages: the first group after an idle gap can see a clock ramp
                hv.timer_start()
                for _ in range(reps):
                    fn()
                m = hv.timer_stop_ms() / reps
                ms = m if ms is None else min(ms, m)
            t[name] = t.get(name, 0.0) + ms
            cnt[name] = cnt.get(name, 0) + 1
        return t, cnt

    def outputs(self):
        """every result buffer of the step: {name: (device tensor, numpy dtype of its values)} -- the tensors hold uint16 / uint32 values as
        int16 / int32 bits (Havoc.zeros)"""
        dt, i16, i32, u32 = self.wl.dtype, np.int16, np.int32, np.uint32
        ime_name, ime = ("sad4", self.o_sad4) if self.ime_range is None else ("sad_surface", self.o_surf)
        out = {ime_name: (ime, i32), "sad": (self.o_sad, i32), "satd_inter": (self.o_satd, i32), "pred": (self.pred, dt), "cpred": (self.cpred, dt), "bi": (self.bi, dt),
               "cbi": (self.cbi, dt), "sbi": (self.sbi, dt)}
        for log2, g in self.intra.items():
            out[f"intra{log2}"] = (g["dst"], dt)
        for log2, g in self.isearch.items():
            out[f"intra_satd35_{log2}"] = (g["cost"], i32)
        for c, g in (self.subpel_planes if self.use_planes else self.subpel).items():
            out["subpel_" + ("x".join(map(str, c)) if isinstance(c, tuple) else str(c))] = (g["cost"], i32)
        for (log2, tr), g in self.tu.items():
            for k, d in (("res", i16), ("coef", i16), ("level", i16), ("deq", i16), ("rec", dt), ("ossd", u32), ("ossd_x", u32)):
                out[f"tu{log2}_{tr}_{k}"] = (g[k], d)
        out["recon_luma"] = (self.luma[3 * self.wl.plane_len:], dt)
        out["recon_chroma"] = (self.chroma[3 * self.wl.cplane_len:], dt)
        for (comp, log2), g in self.recon.items():
            out[f"recon_{comp}{log2}_ssd"] = (g["ssd"], u32)
        return out

    def checksum(self):
        """a checksum of checksums over every result buffer (size-independent parity property; see tests)"""
        import torch
        acc = 0
        for b, _ in self.outputs().values():
            acc = (acc * 1000003 + int(b.to(torch.int64).sum().item())) & 0xFFFFFFFFFFFF
        return acc

    def recon_checksum(self):
        """checksum of the reconstructed picture proper (Y, Cb, Cr without the padding: only reference pictures are padded, so a
        non-reference picture's border holds whatever the context reconstructed before): what a later picture predicts from"""
        import torch
        wl = self.wl
        pl, cpl = wl.plane_len, wl.cplane_len
        acc = 0
        for b, st_, pad, w, h in ((self.luma[3 * pl:4 * pl], wl.stride, 96, wl.width, wl.height),
                                  (self.chroma[3 * cpl:4 * cpl], wl.cstride, 48, wl.width // 2, wl.height // 2),
                                  (self.chroma[4 * cpl:5 * cpl], wl.cstride, 48, wl.width // 2, wl.height // 2)):
            v = b.view(-1, st_)[pad:pad + h, pad:pad + w].to(torch.int64)
            acc = (acc * 1000003 + int(v.sum().item()) * 31 + int((v[::3, ::5] * 7).sum().item())) & 0xFFFFFFFFFFFF
        return acc


class FramePipeline:
    """The frame-parallel step loop (N > 1, or --exchange): time slot t of the DagSchedule.

    compute stream k  : [wait arrived(L0), arrived(L1)] [mirror -> picture store copies] [the picture's graph] [pad] [stage]
    exchange stream   : [wait refs_copied(t), staged(t)] [broadcast of every reference picture of slot t] [record arrived(s)]

    A picture's kernels read their references out of the DPB mirror (copied into the store the captured graph addresses),
    so its results depend on what the references' owners reconstructed; it starts only after the broadcast events of its
    references' mirror slots.  A mirror slot is overwritten (owner's stage, or an incoming broadcast) only after every
    ref copy issued so far on this rank: `refs_copied` events."""

    def __init__(self, torch, dist, exch, contexts, rank, comm, lanes, poc_checksums=False):
        self.torch, self.dist, self.exch, self.ctx, self.rank, self.comm, self.lanes = torch, dist, exch, contexts, rank, comm, lanes
        self.count = 0                    # pictures this rank has worked on -> which context the next one uses
        self.arrived = {}                 # DPB slot -> event recorded after its latest broadcast
        self.staged_at = {}               # DPB slot -> event recorded after THIS rank staged its own reconstruction there
        self.last_copy = [None] * len(contexts)   # per compute stream: event after its latest ref copy
        self.poc_checksums = {} if poc_checksums else None
        self.pictures = 0

    def slot(self, t):
        torch, exch = self.torch, self.exch
        pic = exch.picture_of(t)
        staged = None
        if pic is not None:
            k = self.count % len(self.ctx)
            self.count += 1
            self.pictures += 1
            compute, hv, wl, dev, graph = self.ctx[k]
            pl, cpl = wl.plane_len, wl.cplane_len
            if pic.refs:
                s0, s1 = exch.refs(pic)
                for sl, ref_poc in {(s0, pic.l0), (s1, pic.l1)}:
                    # a reference this rank encoded itself (the anchor chain) is in the mirror once it is staged; one from
                    # another rank once its broadcast has landed
                    local = exch.schedule.rank_of.get(ref_poc) == self.rank and sl in self.staged_at
                    ev = self.staged_at[sl] if local else self.arrived.get(sl)
                    if ev is not None:
                        compute.wait_event(ev)
                with torch.cuda.stream(compute):
                    # references come from the mirror: L0 / L1 luma into store planes 1 / 2 and phase-plane slot 0 of
                    # each reference, Cb of L0 / L1 into the chroma store (one fused copy launch)
                    dst = [dev.luma[pl:2 * pl], dev.luma[2 * pl:3 * pl], dev.chroma[cpl:2 * cpl], dev.chroma[2 * cpl:3 * cpl]]
                    src = [exch.dpb_luma[s0], exch.dpb_luma[s1], exch.dpb_cb[s0], exch.dpb_cb[s1]]
                    if dev.use_planes:
                        dst += [dev.planes[0:pl], dev.planes[16 * pl:17 * pl]]
                        src += [exch.dpb_luma[s0], exch.dpb_luma[s1]]
                    torch._foreach_copy_(dst, src)
                ev = torch.cuda.Event()
                ev.record(compute)
                self.last_copy[k] = ev
            else:
                with torch.cuda.stream(compute):   # no references (IDR): the synthetic ones the context was built with
                    dst = [dev.luma[pl:3 * pl], dev.chroma[cpl:3 * cpl]]
                    src = list(dev.init_refs)
                    if dev.use_planes:
                        dst += [dev.planes[0:pl], dev.planes[16 * pl:17 * pl]]
                        src += [dev.init_refs[0][:pl], dev.init_refs[0][pl:]]
                    torch._foreach_copy_(dst, src)
            if graph is not None:
                hv.graph_launch(graph)
            else:
                dev.step(self.lanes)
            if pic.is_reference:
                # the owner pads its reconstruction (Padding::padBlock after the loop filter, turing/TaskDeblock.cpp:151-159)
                # before it becomes a reference on every rank
                hv.pad_block_d(dev.luma, 3 * pl + 96 * wl.stride + 96, wl.width, wl.height, wl.stride, 96)
                hv.pad_block_d(dev.chroma, 3 * cpl + 48 * wl.cstride + 48, wl.width // 2, wl.height // 2, wl.cstride, 48)
                hv.pad_block_d(dev.chroma, 4 * cpl + 48 * wl.cstride + 48, wl.width // 2, wl.height // 2, wl.cstride, 48)
                for j, ev in enumerate(self.last_copy):      # the mirror slot being staged into may still be read by a
                    if ev is not None and j != k:            # ref copy of the other picture in flight
                        compute.wait_event(ev)
                prev = self.arrived.get(exch.slot_of(pic.poc))   # the slot's previous picture: its broadcast (which this rank
                if prev is not None:                             # may have been the root of) must be over before it is overwritten
                    compute.wait_event(prev)
                with torch.cuda.stream(compute):
                    exch.stage(t, (dev.luma[3 * pl:4 * pl], dev.chroma[3 * cpl:4 * cpl], dev.chroma[4 * cpl:5 * cpl]))
                staged = torch.cuda.Event()
                staged.record(compute)
                self.staged_at[exch.slot_of(pic.poc)] = staged
            if self.poc_checksums is not None:
                hv.sync()
                self.poc_checksums[pic.poc] = dev.recon_checksum()
        for ev in self.last_copy:          # incoming broadcasts overwrite mirror slots: behind every ref copy issued so far
            if ev is not None:
                self.comm.wait_event(ev)
        if staged is not None:
            self.comm.wait_event(staged)
        if exch.plan is not None:          # --bands: the same bytes in CTU-row bands (three broadcasts per band), a band's rows usable as soon as they land
            for b in range(exch.plan.n_bands):
                exch.send_band(t, b)
        else:
            exch.send(t)
        for src in range(exch.world):
            q = exch.picture_of(t, src)
            if q is not None and q.is_reference:
                ev = torch.cuda.Event()
                ev.record(self.comm)
                self.arrived[exch.slot_of(q.poc)] = ev
