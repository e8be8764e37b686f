// One leaf node of the fast BVH4 traversal: the statements of bvh_run's leaf branch, included there
// and in leaf_node_visit (kernel.hip), which the quad tail mode runs on one lane of a quad. A text
// fragment rather than a function: bvh_run's instances compile to the same code as before the
// fragment was shared (as an inlined function the all-features and 3-wave instances allocated
// registers differently). Names it uses from its context: S, delta, lnode, onx, ony, onz, leaf_boxes,
// tmax_entry, r, inv, tmin, mode; it updates closest, best_rank, hit_code, any.
            // The 1-2 leaf children of ONE reference BVH2 node, left then right,
            // and that node's result formed exactly like bvh.rs:377-414: the left
            // leaf is tested with the BVH's entry t_max, the right one with the
            // left hit's t (t_max_for_right), and `if left.t < right.t {left} else
            // {right}`. This matters for f64 spheres: sphere.rs compares its root
            // against the f32 t_max before rounding t to f32, so a sphere whose
            // rounded t equals another candidate's passes or fails depending on
            // which t_max it saw. The node result then joins (closest, DFS rank)
            // like the tree-min does.
            const uint32_t nbo = (lnode & ~rtdev::kLeafNodeFlag) * (rtdev::kBvhNodeF4 * 16u);  // node byte offset
            const f4* nd = S.nodes;
            const float2 nx2 = ld2_at(nd, nbo + onx), ny2 = ld2_at(nd, nbo + ony), nz2 = ld2_at(nd, nbo + onz),
                         fx2 = ld2_at(nd, nbo + (onx ^ 48u)), fy2 = ld2_at(nd, nbo + (ony ^ 80u)),
                         fz2 = ld2_at(nd, nbo + (onz ^ 112u)), chs = ld2_at(nd, nbo + 96u), rks = ld2_at(nd, nbo + 112u);
            float tmr = tmax_entry, nt = 0.0f;
            bool nh = false;
            uint32_t ncode = 0u, nrank = 0u;
            const uint32_t nleaf = __float_as_uint(chs.y) == rtdev::kChildEmpty ? 1u : 2u;
            float llo[2] = {-kInf, -kInf}, lhi[2] = {kInf, kInf};
            if (leaf_boxes) leaf_intervals2_nf(nx2, ny2, nz2, fx2, fy2, fz2, r, inv, delta, llo, lhi);
            for (uint32_t k = 0; k < nleaf; ++k) {
                const uint32_t lcode = __float_as_uint(k ? chs.y : chs.x), rank = __float_as_uint(k ? rks.y : rks.x);
#ifdef RT_LEAF_AUDIT
                const float2 bx0 = ld2(S.nodes + nbo / 16u, 0), by0 = ld2(S.nodes + nbo / 16u, 1),
                             bz0 = ld2(S.nodes + nbo / 16u, 2), bx1 = ld2(S.nodes + nbo / 16u, 3),
                             by1 = ld2(S.nodes + nbo / 16u, 4), bz1 = ld2(S.nodes + nbo / 16u, 5);
                const float x0 = k ? bx0.y : bx0.x, y0 = k ? by0.y : by0.x, z0 = k ? bz0.y : bz0.x;
                const float x1 = k ? bx1.y : bx1.x, y1 = k ? by1.y : by1.x, z1 = k ? bz1.y : bz1.x;
#endif
                // the right leaf can only matter if t <= min(closest, left t)
                const float bound = tmr < closest ? tmr : closest;
                if (!leaf_boxes || leaf_interval_may_hit(k ? llo[1] : llo[0], k ? lhi[1] : lhi[0], tmin, bound)) {
                    PROF_T0(pl);
                    // Only candidates whose f32 t can tie or beat closest matter, so
                    // the test may use min(t_max, nextup(closest)): a root in
                    // (closest, nextup] is still judged against the reference's own
                    // t_max, anything beyond rounds above closest and loses anyway.
                    const float cap = closest < kInf ? __uint_as_float(__float_as_uint(closest) + 1u) : kInf;
                    float c = tmr < cap ? tmr : cap;
                    uint32_t code = 0u;
                    const RayD q = to_d(r);  // f64 ray for sphere leaves, rebuilt here rather than kept live
                    ABLATE(kAbLeaf2, float c2 = c; uint32_t h2 = 0u;
                           if (leaf_hit<kF>(S, lcode, r, q, tmin, c2, h2) && h2 == 0x7fffffffu) c = -1.0f;);
                    // cube sides from the ray's reciprocals (side_t_rcp) except in the triangle preset,
                    // whose instance lost 1.6% to the extra code (C3 +2%; uniform_entries_ab.log)
                    bool hit;
                    if constexpr (kLeafEmbed<kF>) {
                        const uint32_t ltype = rtdev::leaf_type(lcode);
                        // leaf k's lane of rows 0-6 (the node's line, just fetched; the address needs
                        // no record index, so the loads do not wait on the child row)
                        const uint32_t lo = nbo + 4u * k;
                        if (ltype == rtdev::kLeafSphere) {  // (cx, cy, cz, r) in lane 2 + k of rows 0, 1, 2, 6
                            const f4 sp{ld1_at(nd, lo + 8u), ld1_at(nd, lo + 24u), ld1_at(nd, lo + 40u), ld1_at(nd, lo + 104u)};
                            float ts;
                            hit = sphere_t(sp, q, tmin, c, ts);
                            if (hit) {
                                c = ts;
                                code = lcode;
                            }
                        } else if (ltype == rtdev::kLeafCube) {  // its leaf box (lane k of rows 0-5) is its bounds
                            hit = cube_hit<(kF & kFTri) == 0u>(S, rtdev::leaf_index(lcode), ld1_at(nd, lo), ld1_at(nd, lo + 16u),
                                                               ld1_at(nd, lo + 32u), ld1_at(nd, lo + 48u), ld1_at(nd, lo + 64u),
                                                               ld1_at(nd, lo + 80u), r, inv, tmin, c, code);
                        } else {
                            hit = leaf_hit<kF, (kF & kFTri) == 0u, false, true>(S, lcode, r, q, tmin, c, code, inv);
                        }
                    } else {
                        hit = leaf_hit<kF, (kF & kFTri) == 0u>(S, lcode, r, q, tmin, c, code, inv);
                    }
                    if (hit) {
                        // cube faces rank + 0..5 (the face leaf_hit's list walk kept)
                        const uint32_t rk = rank + (rtdev::leaf_type(lcode) == rtdev::kLeafCube
                                                        ? rtdev::leaf_index(code) - rtdev::leaf_index(lcode)
                                                        : 0u);
                        if (!nh || !(nt < c)) {
                            nh = true;
                            nt = c;
                            ncode = code;
                            nrank = rk;
                        }
                        tmr = c;
                    }
                    PROF_ADD(kPrLeafTest, pl);
                } else {
                    LEAF_AUDIT(lcode, rank, x0, y0, z0, x1, y1, z1);
                }
            }
            if (nh && (nt < closest || (nt == closest && nrank > best_rank))) {
                closest = nt;
                best_rank = nrank;
                hit_code = ncode;
                any = true;
            }
