/* k_fast_group_lm.h -- part of hip_backend.hip: the evaluation of one row group in fast_voice (k_fast_voice.h) in the lane-major
 * form (SPLIT 3: the INNER build's groups between, closed-form phases, no segment edge in the group). The group's 64 T frames are
 * the same as k_fast_group.h's, [cg GF - H, cg GF - H + 64 T); relative frame j = l T + k lies in lane l, register k, where the
 * row-major form has j = 64 k + l. A frame's neighbour before is then register k - 1 of the same lane, and only register 0 reads
 * lane l - 1's register T - 1: one DPP move per dword of a differentiator per group, where the row-major form's later rows take two
 * per register (prev_of there) -- 5.3 of the build's 31.7 vector instructions per operator-sample (profiles/census/).
 * The block buffer is T registers of the lane (blk): where the row-major form keeps element (k, l) at off + 64 k + l in LDS, here
 * lane l both writes and reads it, and the launch only takes segments whose voices share ONE buffer (launch_plan.h:
 * plan_closed_form), so every *_off that is not ~0u names that block. The launch's LDS holds the tables and nothing else.
 * The arithmetic and its order are k_fast_group.h's with EDGE false, SCAN 0, REPAIR false, CUB false; only what reaches a frame's
 * neighbour differs. In scope: everything fast_voice has defined up to its row-group loop, plus cg.
 * WONLY (round 11, fast_voice's flag): the same file as the instantiation for banks of wave oscillators with constant amplitude --
 * every branch such a step does not take is compiled out (`!WONLY && ...`), and the general instantiation's code is what it was. */
		const int j0 = l * T;                              /* this lane's first frame of the group, relative */
		const int t0 = (int)(cg * GF) - (int)H + j0;       /* ... and in the segment: register k holds frame t0 + k */
		/* which registers hold frames of the group's own (lead-in: j < H -- the first lanes' first registers): bit k */
		const uint32_t om = ((1u << T) - 1u) & ~((1u << min(max((int)H - j0, 0), T)) - 1u);
		/* the frame before: the register before; for register 0 lane l - 1's last (lane 0: zero; frame 0 is lead-in) */
		auto prev32 = [&](const uint32_t *x, int k) -> uint32_t { return k > 0 ? x[k - 1] : lane_prev(x[T - 1]); };
		auto prev64 = [&](const double *x, int k) -> double { return k > 0 ? x[k - 1] : lane_prev(x[T - 1]); };
		/* a voice row's frames of this lane: T consecutive floats. 16-byte stores where the group starts on a multiple of four frames
		 * (then so does every lane's run, T being one), for the quads the lane owns whole; dword stores elsewhere */
		const bool quads = ((cg * GF - H) & 3u) == 0;
		/* (the tests on the mask at the stores, not hoisted out of the step loop: as lane masks they took two scalar registers each) */
		auto store_row = [&](float *row, const float *x, const bool nt) {
			uint32_t o = om;
			asm volatile("" : "+v"(o));
			if (quads) {
#pragma unroll
				for (int q = 0; q < T / 4; ++q) {
					const uint32_t oq = (o >> (4 * q)) & 15u;
					if (oq == 15u) {
						const fk_f32x4 v4 = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
						fk_f32x4 *p = (fk_f32x4 *)(row + t0 + 4 * q);
						if (nt) FK_VSTORE(p, v4); else *p = v4;
					} else if (oq != 0u) {
#pragma unroll
						for (int u = 0; u < 4; ++u)
							if ((oq >> u) & 1u) { if (nt) FK_VSTORE(&row[t0 + 4 * q + u], x[4 * q + u]); else row[t0 + 4 * q + u] = x[4 * q + u]; }
					}
				}
			} else {
#pragma unroll
				for (int k = 0; k < T; ++k)
					if ((o >> k) & 1u) { if (nt) FK_VSTORE(&row[t0 + k], x[k]); else row[t0 + k] = x[k]; }
			}
		};
		uint32_t held_rows = 0; /* which of the group's first owned frames unresolved holds spoil (bit j: owned frame j, as k_fast_group.h) */
		bool held_far = false;  /* ... or something the repair pass cannot put right */
		/* the block buffer: this lane's T values, written by one step and read by a later one of the same group (nothing is carried
		 * from group to group: a group evaluates all its steps from scratch) */
		float blk[T];
		for (uint32_t si = 0; si < n_fsteps; ++si) {
			const FastStep f = load_step_uniform(fsteps + si);
			const uint32_t kind = f.kind & 0xff;
			const uint32_t flags = (f.kind >> 8) & 0xff;
			/* (the step's own copy of t0: t0 + 1 ... t0 + T - 1, which only the ramps, N and R read, were computed ahead of the step
			 * loop and held in T - 1 registers across it -- registers the block now needs) */
			int t0s = t0;
			if (!WONLY) asm volatile("" : "+v"(t0s)); /* (the wave-only instantiation has no reader of it) */
			{
				/* A step that needs a second block -- a buffer beyond the first, PM beside FPM, a range list's blend or envelope, a pan
				 * block -- is not this form's. The host does not send such a segment here (launch_plan.h: plan_closed_form); should a
				 * step say so all the same, the voice goes to the block loop, as with holds the repair pass cannot put right. */
				/* (off + 1: 0 none, 1 the first buffer, more another one -- in integers: as booleans these tests became vector code) */
				const uint32_t o1 = f.out_off + 1u, p1 = f.pm_off + 1u, q1 = f.fpm_off + 1u, a1 = f.amp_off + 1u;
				uint32_t two = 0;
				if (WONLY) {
					/* The wave-only instantiation (k_fast_voice.h: fast_kernel's WONLY) holds W oscillator steps with one amplitude
					 * value -- and the same step standing still (k_decode.h makes it a constant source, type OT_AMP) --, the plain
					 * combine and ST_VOICE. Anything else -- an amplitude block or ramp, a layered or enveloped combine,
					 * frequency-scaled PM, an R or N operator, a line, a blend -- and the voice goes to the block loop. The host
					 * sends no such segment here (launch_plan.h: FastPlan.inner_wonly). */
					/* (the type in integers too: OT_WAVE and OT_AMP are the two values without a bit beside OT_WAVE's) */
					static_assert(OT_AMP == 0 && OT_WAVE == 2, "the types as bits");
					const uint32_t ty = f.type & 0xff & ~(uint32_t)OT_WAVE;
					if (kind == ST_OSC) two = o1 | p1 | ((a1 | q1 | (flags & (SF_WAVE_ENV | SF_LAYER)) | (f.ramp & 1u) | ty) << 1);
					else if (kind == ST_VOICE) two = o1 | (p1 << 1);
					else two = 2u;
				} else
				if (kind == ST_OSC) two = o1 | a1 | (p1 + q1) | (flags & SF_WAVE_ENV);
				else if (kind == ST_LINE) two = o1;
				else if (kind == ST_VOICE) two = o1 | (p1 << 1);
				else if (kind == ST_LERP) two = 2u;
				if (two > 1u) { zero_acc = 1; continue; }
			}
			if (kind == ST_OSC) {
				const uint32_t type = f.type & 0xff;
				const bool layer = (flags & SF_LAYER) != 0;
				const bool to_voice = ((f.kind >> 16) & OX_VOICE) != 0;
				float s[T];
				if (type == OT_WAVE) {
					const bool has_pm = f.pm_off != ~0u, has_fpm = !WONLY && f.fpm_off != ~0u; /* (WONLY: no frequency-scaled PM -- it would keep pm_offset32 and the frequency registers in the general path) */
					/* this operator's values are defined from relative frame p_min on */
					const int p_min = (int)H - (int)(f.kind >> 24) + 1;
					/* which of this lane's registers hold frames the operator defines (j >= p_min): bit k -- per-lane masks, where
					 * arrays of flags took a lane-mask register pair each */
					const int nd = min(max(p_min - j0, 0), T);
					const uint32_t dm = ((1u << T) - 1u) & ~((1u << nd) - 1u);
					bool done = false;
					if (FK_COMMON && f.tab >= 0 && !has_fpm && !(f.ramp & 2)) {
						/* the common case, straight-line: table in LDS, plain PM or none */
						uint32_t ph[T];
						bool ok = true;
						if (WONLY && FK_LM_WONLY_ADD3) {
							/* (round 11) A PM operator's phase in ONE add a sample: base + k inc + offset, a three-operand add whose
							 * second operand, the multiple of the wave-uniform increment, is a scalar register -- where acc += inc and
							 * then ph += offset are two vector adds a sample. Mod 2^32 either way: the same phases. Without PM one
							 * add a sample, as before. */
							const uint32_t base = f.phase0 + f.inc * (uint32_t)(t0 + 1);
							if (has_pm) {
								bool big = false;
#pragma unroll
								for (int k = 0; k < T; ++k) big |= !(fabsf(blk[k]) < 0x1p20f);
								ok = !__any(big);
#pragma unroll
								for (int k = 0; k < T; ++k) ph[k] = base + (uint32_t)k * f.inc + rint32w_p31_small(blk[k]);
							} else { /* (as a sum of k inc here too the compiler made 64-bit multiply-adds of most of them) */
								uint32_t acc = base;
#pragma unroll
								for (int k = 0; k < T; ++k) { ph[k] = acc; acc += f.inc; }
							}
						} else {
							uint32_t acc = f.phase0 + f.inc * (uint32_t)(t0 + 1);
#pragma unroll
							for (int k = 0; k < T; ++k) { ph[k] = acc; acc += f.inc; }
						}
						if (!(WONLY && FK_LM_WONLY_ADD3) && has_pm) {
							float pm[T];
							bool big = false;
#pragma unroll
							for (int k = 0; k < T; ++k) {
								pm[k] = blk[k];
								big |= !(fabsf(pm[k]) < 0x1p20f);
							}
							ok = !__any(big);
#pragma unroll
							for (int k = 0; k < T; ++k) ph[k] += rint32w_p31_small(pm[k]);
						}
						if (ok) {
							const uint32_t ltab = tabs + (uint32_t)f.tab * FkTab<WIDE>::BYTES;
							/* The Hermite values in frame order, handed to `sink` two samples at a time (k of the first, the two values).
							 * FK_LM_AHEAD: a window of table entries, a pair of samples to a slot -- the gathers of the pairs ahead are
							 * issued, then (a fence for the compiler's scheduler, no instruction) this pair's arithmetic, which the sink's
							 * FK_LM_PIN ends: its waits count only its own entries' reads, and the later pairs' stay in flight across it.
							 * Left to itself the compiler puts each pair's gather right ahead of its polynomials and waits there, six
							 * times per operator and group. */
							static_assert(T % 2 == 0, "pairs of samples");
							auto hermite = [&](auto &&sink) {
#if FK_LM_AHEAD > 0
								constexpr int NP2 = T / 2, A = FK_LM_AHEAD < NP2 ? FK_LM_AHEAD : NP2 - 1, NS = A + 1;
								FkHerp q[2 * NS];
#pragma unroll
								for (int p = 0; p < A; ++p) {
									q[2 * p] = fk_entry<WIDE, TAB0, true>(ltab, ph[2 * p]);
									q[2 * p + 1] = fk_entry<WIDE, TAB0, true>(ltab, ph[2 * p + 1]);
								}
#pragma unroll
								for (int p = 0; p < NP2; ++p) {
									if (p + A < NP2) {
										const int sl = (p + A) % NS;
										q[2 * sl] = fk_entry<WIDE, TAB0, true>(ltab, ph[2 * (p + A)]);
										q[2 * sl + 1] = fk_entry<WIDE, TAB0, true>(ltab, ph[2 * (p + A) + 1]);
									}
									__builtin_amdgcn_sched_barrier(0);
									const int sl = p % NS;
									sink(2 * p, fk_poly(q[2 * sl], ph[2 * p]), fk_poly(q[2 * sl + 1], ph[2 * p + 1]));
								}
#define FK_LM_PIN(...) asm volatile("" : __VA_ARGS__) /* (the values are computed here, ahead of the next fence) */
#else
#pragma unroll
								for (int k = 0; k < T; k += 2)
									sink(k, fk_poly(fk_entry<WIDE, TAB0>(ltab, ph[k]), ph[k]), fk_poly(fk_entry<WIDE, TAB0>(ltab, ph[k + 1]), ph[k + 1]));
#define FK_LM_PIN(...) ((void)0)
#endif
							};
#if FK_LM_ONE_PHASE_SET
							/* A sample's differentiator right behind its polynomial: it reads ph[k] and ph[k - 1] there, so the phases' last
							 * use is inside the Hermite loop and they live in one register set (as two loops the compiler kept a second copy
							 * for the differentiators: 6-18 moves per operator and group and twelve registers), and of the Hermite values
							 * only the one before and the lane's first are kept, not T. Register 0's output comes last: its frame before
							 * is lane l - 1's register T - 1. The same operations on the same operands as the two loops. */
							double I0 = 0., Ip = 0.;
							if (FK_CONSTD && !has_pm && f.inc != 0) {
								/* unmodulated: every phase step is inc, one division serves all */
								const double x = (double)div_f32_normal(f.diff_scale, (float)(int32_t)f.inc);
								hermite([&](const int k, const double Ia, const double Ib) {
									if (k == 0) I0 = Ia;
									else s[k] = (float)((Ia - Ip) * x + (double)f.diff_offset);
									s[k + 1] = (float)((Ib - Ia) * x + (double)f.diff_offset);
									Ip = Ib;
									if (k == 0) FK_LM_PIN("+v"(I0), "+v"(s[1]));
									else FK_LM_PIN("+v"(s[k]), "+v"(s[k + 1]));
								});
								s[0] = (float)((I0 - lane_prev(Ip)) * x + (double)f.diff_offset);
								done = true;
							} else {
								/* a phase step of zero anywhere: the unsigned minimum of the steps (v_min_u32, k_fast_group.h) */
								uint32_t dmin = 0xffffffffu;
								uint32_t pp = lane_prev(ph[T - 1]);
								asm("" : "+v"(pp)); /* (keeps the DPP move a move: k_fast_group.h) */
								const int32_t d0 = (int32_t)(ph[0] - pp);
								/* (this branch takes the phases through an empty asm: the two copies of the Hermite loop then share no
								 * expression, and the compiler does not compute all T addresses and fractions -- 36 registers -- ahead of
								 * the branch for both) */
#pragma unroll
								for (int k = 0; k < T; ++k) asm volatile("" : "+v"(ph[k]));
								double x0 = 0.;
								hermite([&](const int k, const double Ia, const double Ib) {
									/* wosc_diff (sau_dev_math.h) on the two samples, their divisions as one packed sequence */
									const int32_t da = k == 0 ? d0 : (int32_t)(ph[k] - ph[k - 1]), db = (int32_t)(ph[k + 1] - ph[k]);
									dmin = min(dmin, min((uint32_t)da, (uint32_t)db));
									const fk_f32x2 dv = {(float)da, (float)db};
									const fk_f32x2 x = fk_div_diff_scale2(f.diff_scale, dv);
									if (k == 0) { I0 = Ia; x0 = (double)x.x; }
									else s[k] = (float)((Ia - Ip) * (double)x.x + (double)f.diff_offset);
									s[k + 1] = (float)((Ib - Ia) * (double)x.y + (double)f.diff_offset);
									Ip = Ib;
									if (k == 0) FK_LM_PIN("+v"(I0), "+v"(x0), "+v"(s[1]), "+v"(dmin));
									else FK_LM_PIN("+v"(s[k]), "+v"(s[k + 1]), "+v"(dmin));
								});
								s[0] = (float)((I0 - lane_prev(Ip)) * x0 + (double)f.diff_offset);
								/* (a zero: the general path below, which starts from the step again, tells zeros on defined frames from
								 * those on lead-in frames, which may have any, and computes every other frame as here -- the phases are
								 * not kept for that test) */
								done = !__any(dmin == 0u);
							}
#else
							double Is[T];
							hermite([&](const int k, const double Ia, const double Ib) { Is[k] = Ia; Is[k + 1] = Ib; FK_LM_PIN("+v"(Is[k]), "+v"(Is[k + 1])); });
							if (FK_CONSTD && !has_pm && f.inc != 0) {
								/* unmodulated: every phase step is inc, one division serves all */
								const double x = (double)div_f32_normal(f.diff_scale, (float)(int32_t)f.inc);
#pragma unroll
								for (int k = 0; k < T; ++k)
									s[k] = (float)((Is[k] - prev64(Is, k)) * x + (double)f.diff_offset);
								done = true;
							} else {
								/* a phase step of zero anywhere: the unsigned minimum of the steps (v_min_u32, k_fast_group.h), then
								 * -- rarely -- which of the zeros fall on defined frames (lead-in frames may have any) */
								uint32_t dmin = 0xffffffffu;
#pragma unroll
								for (int k = 0; k < T; ++k) {
									uint32_t pp = prev32(ph, k);
									if (k == 0) asm("" : "+v"(pp)); /* (keeps the DPP move a move: k_fast_group.h) */
									const int32_t d = (int32_t)(ph[k] - pp);
									dmin = min(dmin, (uint32_t)d);
									s[k] = wosc_diff(Is[k], prev64(Is, k), d, f.diff_scale, f.diff_offset);
								}
								done = true;
								if (__any(dmin == 0u)) {
									uint32_t hz = 0;
#pragma unroll
									for (int k = 0; k < T; ++k) hz |= ph[k] == prev32(ph, k) ? 1u << k : 0u;
									done = !__any((hz & dm) != 0u);
								}
							}
#endif
#undef FK_LM_PIN
						}
					}
					if (!done) {
						uint32_t ph[T];
						double Is[T];
						float fv[T]; /* frequency per frame (freq-scaled PM reads it) */
						{
							uint32_t inc = f.inc;
#if FK_LM_ONE_PHASE_SET
							/* (an increment the compiler cannot see through: these phases are computed here, where the rare step needs
							 * them. As the common path's own expressions they were computed once ahead of both paths and the T
							 * unmodulated phases held in registers across the common path for this one) */
							asm volatile("" : "+s"(inc));
#endif
							uint32_t acc = f.phase0 + inc * (uint32_t)(t0 + 1);
#pragma unroll
							for (int k = 0; k < T; ++k) { ph[k] = acc; acc += inc; fv[k] = f.fc; }
						}
						if (has_pm && !has_fpm) {
							float pm[T];
							bool big = false;
#pragma unroll
							for (int k = 0; k < T; ++k) {
								pm[k] = blk[k];
								big |= !(fabsf(pm[k]) < 0x1p20f);
							}
							if (!__any(big)) {
#pragma unroll
								for (int k = 0; k < T; ++k) ph[k] += rint32w_p31_small(pm[k]);
							} else {
#pragma unroll
								for (int k = 0; k < T; ++k) ph[k] += rint32w_p31(pm[k]);
							}
						} else if (has_fpm) {
#pragma unroll
							for (int k = 0; k < T; ++k) ph[k] += pm_offset32(false, true, 0.f, blk[k], fv[k]);
						}
						if (f.tab >= 0) {
							const uint32_t ltab = tabs + (uint32_t)f.tab * FkTab<WIDE>::BYTES;
#pragma unroll
							for (int k = 0; k < T; ++k) Is[k] = fk_poly(fk_entry<WIDE, TAB0>(ltab, ph[k]), ph[k]);
						} else {
							const uint32_t wave = (f.type >> 8) & 0xff;
							const HerpC23 *g23 = P.g_c23 + (size_t)wave * WAVE_LEN;
							const HerpC01 *g01 = P.g_c01 + (size_t)wave * WAVE_LEN;
#pragma unroll
							for (int k = 0; k < T; ++k) {
								const uint32_t ind = ph[k] >> SLEN_BITS;
								Is[k] = herp_poly(g23[ind], g01[ind], ph[k]);
							}
						}
						uint32_t hz = 0; /* registers with a phase step of zero: bit k */
						if (FK_CONSTD && !has_pm && !has_fpm && f.inc != 0) {
							/* unmodulated: every phase step is inc, one division serves all */
							const double x = (double)div_f32_normal(f.diff_scale, (float)(int32_t)f.inc);
#pragma unroll
							for (int k = 0; k < T; ++k) {
								const double pIs = prev64(Is, k);
								s[k] = (float)((Is[k] - pIs) * x + (double)f.diff_offset);
							}
						} else {
#pragma unroll
							for (int k = 0; k < T; ++k) {
								const uint32_t pph = prev32(ph, k);
								const double pIs = prev64(Is, k);
								const int32_t d = (int32_t)(ph[k] - pph);
								hz |= d == 0 ? 1u << k : 0u;
								s[k] = wosc_diff(Is[k], pIs, d, f.diff_scale, f.diff_offset);
							}
						}
						uint32_t held = hz & dm;
						if (__any(held != 0u)) {
							/* dphase == 0: the differentiator holds its previous output (wosc.h:251-252). In frame order: a pass
							 * over the lane's registers, then -- for runs that cross from one lane into the next -- lane l - 1's
							 * last register, and again the pass, until nothing changes. A run that reaches back to the operator's
							 * first defined frame stays: the repair pass's (below). */
							uint32_t src = dm & ~held; /* holds a defined output to copy from */
							auto in_lane = [&]() {
#pragma unroll
								for (int k = 1; k < T; ++k)
									if (((held >> k) & 1u) && ((src >> (k - 1)) & 1u)) { s[k] = s[k - 1]; held &= ~(1u << k); src |= 1u << k; }
							};
							in_lane();
							for (int it = 0; it < 64; ++it) {
								const float sp = __shfl_up(s[T - 1], 1);
								const uint32_t okp = ((uint32_t)__shfl_up((int)src, 1) >> (T - 1)) & 1u;
								bool changed = false;
								if ((held & 1u) && okp && l > 0) { s[0] = sp; held &= ~1u; src |= 1u; changed = true; in_lane(); }
								if (!__any(changed)) break;
							}
							/* What is left is a run of repeats that begins on the operator's first defined frame, p_min; the hold at
							 * p_min + j spoils the carrier's owned frame j (k_fast_group.h). The repair pass stores the first jm such
							 * frames; a hold further on is not a case for it. */
							const int jm = min(32, 64 - (int)FAST_REPAIR_SHIFT - (int)H);
							if (held) {
								const int j = j0 + (int)__builtin_ctz(held);
								rep[1] = ((uint32_t)(j % 64 - p_min) << 24) | ((uint32_t)(j / 64) << 20) | (si << 12) | (cg & 0xfff); /* debug */
							}
							const int nf = jm + p_min - j0; /* this lane's first register beyond the frames the repair pass stores */
							const bool far = nf <= 0 ? held != 0u : nf < T ? (held >> nf) != 0u : false;
							if (__any(far)) held_far = true;
							if (jm > 0) {
								/* the frames p_min .. p_min + jm - 1 as bits: the first lanes' held registers side by side */
								unsigned long long run = 0;
#pragma unroll
								for (int L = 0; L * T < 64; ++L)
									run |= (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)held, L) << (L * T);
								held_rows |= (uint32_t)((run >> p_min) & ((1ull << jm) - 1ull));
							}
						}
					}
				} else if (!WONLY && type == OT_RASEG) {
					/* rasg.h:165-222 + 692-743: frame t reads the counter cp0 + inc * t (+ PM) */
					const bool rate2x = (f.type >> 17) & 1;
					const float phase_scale = rate2x ? 0x1p31f * 2 : 0x1p31f;
					const RasParams rp = ras_params((uint32_t)f.tab & 0xff, ((uint32_t)f.tab >> 8) & 0xffff,
							f_bits(f.diff_scale), f_bits(f.diff_offset), ((uint32_t)f.tab >> 24) & 0x7f);
					const unsigned long long inc64 = ((unsigned long long)f.prev_phase << 32) | f.inc;
					const unsigned long long cp0 = (unsigned long long)__double_as_longlong(f.prev_Is);
					const bool has_pm = f.pm_off != ~0u, has_fpm = f.fpm_off != ~0u;
#pragma unroll
					for (int k = 0; k < T; ++k) {
						unsigned long long cp = cp0 + inc64 * (unsigned long long)(long long)(t0s + k);
						if (has_pm || has_fpm)
							cp += (unsigned long long)pm_offset(has_pm, has_fpm,
									has_pm ? blk[k] : 0.f,
									has_fpm ? blk[k] : 0.f, f.fc, phase_scale);
						uint32_t cyc;
						float phf;
						ras_split(cp, cyc, phf);
						s[k] = ras_sample(rp, cyc, phf, true, false);
					}
				} else if (!WONLY && type == OT_NOISE) {
					const uint32_t nz = (f.type >> 8) & 0xff;
					const uint32_t n0 = f.phase0;
#pragma unroll
					for (int k = 0; k < T; ++k) {
						const uint32_t n = n0 + (uint32_t)(t0s + k);
						if (nz == NZ_vi) {
							uint32_t s1 = ranfast32(n);
							uint32_t s0 = ranfast32(n - 1);
							s[k] = fscalei((s1 / 2) - (s0 / 2), 0x1p-31f);
						} else if (nz == NZ_bv) {
							int32_t s1 = noise_bv_term(n);
							int32_t s0 = noise_bv_term(n - 1);
							s[k] = (float)(s1 - s0);
						} else {
							s[k] = noise_stateless(nz, n);
						}
					}
				} else { /* OT_AMP (generator.c:517-518: 1), or an oscillator whose output stands still */
#pragma unroll
					for (int k = 0; k < T; ++k) s[k] = f.fc;
				}
				/* amplitude and combine: generator.c:384-440 */
				if (WONLY && FK_LM_WONLY_INPLACE) {
					/* (round 11) one amplitude value and the plain combine, the products written where they go: to the row store
					 * of the step that feeds the voice, else over the block's registers -- whose old values no later code of this
					 * step reads here, where the general instantiation may still layer onto them or read them as amplitudes
					 * and so keeps them beside the new ones */
					if (to_voice) {
						float x[T];
#pragma unroll
						for (int k = 0; k < T; ++k) x[k] = s[k] * f.ac;
						store_row(vrow, x, true);
					} else {
#pragma unroll
						for (int k = 0; k < T; ++k) blk[k] = s[k] * f.ac;
					}
					continue;
				}
				float r[T];
				if (!WONLY && f.amp_off != ~0u) {
#pragma unroll
					for (int k = 0; k < T; ++k) r[k] = blk[k];
				} else if (!WONLY && (f.ramp & 1)) { /* amplitude ramp in progress, sau/line.c:65-281 */
					const FastLine fl = load_line_uniform(flines + si);
#pragma unroll
					for (int k = 0; k < T; ++k) r[k] = fast_line_value(fl, t0s + k);
				} else {
#pragma unroll
					for (int k = 0; k < T; ++k) r[k] = f.ac;
				}
				if (!WONLY && layer) {
#pragma unroll
					for (int k = 0; k < T; ++k) r[k] = mix_combine(blk[k], s[k], r[k], false, true);
				} else {
#pragma unroll
					for (int k = 0; k < T; ++k) r[k] = s[k] * r[k];
				}
				if (to_voice) {
					store_row(vrow, r, true);
				} else {
#pragma unroll
					for (int k = 0; k < T; ++k) blk[k] = r[k];
				}
			} else if (!WONLY && kind == ST_LINE) {
				/* held line: v0 (sau/line.c:435-442) */
				if (f.ramp) {
					FastLine fl;
					fl.goal_len = 0; fl.hold = f.ac; fl.pad = 0;
					fl.sw = sweep_setup(LN_sah, 0.f, 0.f, 0, 1);
					if (f.ramp & 1) fl = load_line_uniform(flines + si);
#pragma unroll
					for (int k = 0; k < T; ++k) blk[k] = fast_line_value(fl, t0s + k);
				} else {
#pragma unroll
					for (int k = 0; k < T; ++k) blk[k] = f.ac;
				}
			} else if (kind == ST_VOICE) { /* generator.c:749-788, the pan one value */
				store_row(vrow, blk, true);
				if (prow) {
					float x[T];
#pragma unroll
					for (int k = 0; k < T; ++k) x[k] = f.pan;
					store_row(prow, x, false);
				}
			}
		}
		if (held_rows || held_far) {
			/* to the repair pass (k_fast_group.h) */
			bool noted = false;
			if (P.repair_on && !held_far && (int)(cg * GF) - (int)H >= (int)FAST_REPAIR_SHIFT) {
				uint32_t at = 0;
				if (l == 0) at = atomicAdd(&rep[0], 1u);
				at = uni(at);
				if (at < FAST_MAX_REPAIR) {
					if (l == 0) {
						rep[2 + 2 * at] = cg;
						rep[3 + 2 * at] = held_rows;
						atomicOr(&P.pass_flags[FAST_MAX_LEVELS], 1u);
						atomicOr(&P.work_count[1], 2u); /* (frames the mixer may have taken early -- k_finish.h: premix_kernel -- change in the repair pass) */
					}
					noted = true;
				}
			}
			if (!noted) zero_acc = 1;
		}
