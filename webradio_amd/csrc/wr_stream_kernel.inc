/*
 * wr_stream_kernel.inc -- k_tuner_stream: the fused per-tuner path as ONE persistent launch fed by a doorbell
 * (included at the end of wr_kernels.hip: it is built from that file's device functions).
 *
 * Reference semantics it keeps: DspBlock::run hands a block's output on within the run() that brought the block
 * (dsp/dspblock.cxx:169-212), the tuner thread swaps a new block in whenever it has one
 * (io/rtlsdrtuner.cxx:265-285).  With one kernel launch per block the GPU pays, per block, what a launch costs
 * INSIDE the kernel: every wave's per-channel state, the NCO tables to LDS, the first windows from HBM (about
 * 3 us before the first tap at C2), and a ragged end in which the last waves run on a part-empty chip -- 4.6 us of
 * a 32 us block.  Here the grid is resident for the whole stream:
 *
 *   workgroups [0, n_ddc)            the DDC waves of k_tuner_ddc's lean loop (ROTATE NCO, NG lane groups per wave: two
 *                                    on ONE channel filter, or one lane group with up to TS = WR_TAPSETS distinct ones,
 *                                    a window copy per filter -- stream_ddc), walking the output frames of block 0, 1,
 *                                    2, ... as ONE sequence -- a wave's units are every wpg-th frame of the STREAM, so the units come out even
 *                                    over the stream, not per block.  Channel IQ goes to a ring of WR_STREAM_RING blocks.
 *   workgroups [n_ddc, n_ddc+n_post) the post stage (post_role: demodulator + audio filter), block by block: block j
 *                                    as soon as all of its channel-IQ rows are out and block j-1's post stage has left
 *                                    its state (the audio filter's history, Demodulator::prev_i/q) behind.
 *                                    The first of them also do the frames of block 0 whose windows reach into the block
 *                                    BEFORE the stream (kept turns and LO values: ddc_body's block-boundary role).
 *   workgroup  n_ddc+n_post          one lane: the bell.  It polls the doorbell in page-locked host memory
 *                                    (WrStreamCtl::ready / stop), copies the descriptors of new blocks to device memory
 *                                    and republishes the count there -- thousands of waves never poll across PCIe.
 *
 * Hand-overs inside the launch follow MI355X_MICROARCH.md "inter-workgroup visibility":
 *   channel IQ   write-through (agent-scope) stores, s_waitcnt vmcnt(0), relaxed agent add on ddc_done[j]; the post
 *                workgroup: ONE lane polls (relaxed agent loads, s_sleep), ONE agent acquire, __syncthreads, plain loads.
 *   post state   plain stores, __syncthreads, lane 0: release fence, s_waitcnt vmcnt(0), relaxed add on post_done[j];
 *                consumer as above.  The last arriver tells the host (WrStreamCtl::done, system scope).
 * Every wait has a deadline (WrStreamArgs::wait_ticks of the constant 100 MHz clock): a wait that runs into it sets
 * WrStreamCtl::err, closes the stream for everybody and the launch ENDS -- an error, never a hung GPU.  The bell closes
 * the stream on its own when the doorbell has been silent for idle_ticks (a caller that synchronises the stream behind
 * the library's back waits that long, no longer).
 *
 * Bits: the lean loop's arithmetic per output frame is k_tuner_ddc's, literally: both call the same functions of
 * wr_kernels.hip -- lean_rec (a lane's recurrences), lean_win (its taps and window buffers; LeanWin::to_lds), rotate_unit
 * (one output frame's taps) and rot_tables_to_lds.  Frames of blocks j >= 1 whose windows reach into block j-1 take
 * the SAME path with the window read from two places -- the step cannot change inside a stream (a setter closes it), so
 * no kept turns are needed -- which is what "bits do not depend on where the block boundaries fall" (DESIGN.md 4)
 * promises; tests/test_gpu_stream.py holds it to that.
 */

__device__ __forceinline__ unsigned int st_rfl(unsigned int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned int st_ld(const unsigned int *p)
{
	return st_rfl(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ unsigned long long st_ld64(const unsigned long long *p)
{
	const unsigned long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return ((unsigned long long)st_rfl((unsigned int)(v >> 32)) << 32) | st_rfl((unsigned int)v);
}
__device__ __forceinline__ unsigned int st_ld_sys(const volatile unsigned int *p)
{
	return st_rfl(__hip_atomic_load((const unsigned int *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
__device__ __forceinline__ void st_st_sys(volatile unsigned int *p, unsigned int v)
{
	__hip_atomic_store((unsigned int *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ unsigned int st_ddc_ready(const WrStreamArgs &S)
{
	return st_rfl((unsigned int)__hip_atomic_load(&S.sdev->progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ unsigned int st_post_ready(const WrStreamArgs &S)
{
	return st_rfl((unsigned int)(__hip_atomic_load(&S.sdev->progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32));
}

/* a wait ran into its deadline: say so, and close the stream for everybody */
__device__ __forceinline__ void stream_fail(const WrStreamArgs &S)
{
	st_st_sys(&S.ctl->err, WR_STREAM_ERR_WAIT);
	__hip_atomic_store(&S.sdev->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* is block `need` there?  Waits until the bell has republished it, or the stream is closed.  `known` = blocks known to
 * be submitted (never falls); `closed`: the stream is closed and `known` is final.  Wave-uniform. */
__device__ __forceinline__ bool stream_wait_ready(const WrStreamArgs &S, unsigned int need, unsigned int &known, bool &closed)
{
	if (need < known)
		return true;
	if (closed)
		return false;
	const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
	unsigned int spins = 0;
	for (;;) {
		const unsigned int r = st_ld(&S.sdev->ready);
		if (r > need) {
			known = r;
			return true;
		}
		if (st_ld(&S.sdev->stop)) {
			/* (the bell publishes the final count BEFORE the stop: read after it, the count is final.  It publishes
			 * counts from 2 on: block 0 is there from the start -- the launch exists because of it) */
			const unsigned int f = st_ld(&S.sdev->ready);
			if (f > known)
				known = f;
			closed = true;
			return known > need;
		}
		if ((++spins & 63u) == 0u) {
			/* the host may leave a stream open for as long as it likes: what must not go silent is the bell, which
			 * stamps WrStreamDev::beat every time round its loop */
			const unsigned long long now = __builtin_amdgcn_s_memrealtime();
			const unsigned long long beat = __hip_atomic_load(&S.sdev->beat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (now - t0 > S.wait_ticks && now >= beat && now - beat > S.wait_ticks) {
				stream_fail(S);
				if (r > known)
					known = r;
				closed = true;
				return false;
			}
		}
		__builtin_amdgcn_s_sleep(20);
	}
}

/* wait until the counter at `p` has reached `target`; false = gave up (deadline, or somebody else's error) */
__device__ __forceinline__ bool stream_wait_count(const WrStreamArgs &S, const unsigned int *p, unsigned int target)
{
	/* (the two halves of WrStreamDev::progress are little-endian words of their own) */
	if (st_ld(p) >= target)
		return true;
	const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
	unsigned int spins = 0;
	for (;;) {
		__builtin_amdgcn_s_sleep(20);
		if (st_ld(p) >= target)
			return true;
		if ((++spins & 63u) == 0u) {
			if (__builtin_amdgcn_s_memrealtime() - t0 > S.wait_ticks) {
				stream_fail(S);
				return false;
			}
			if (st_ld_sys(&S.ctl->err))
				return false;
		}
	}
}

/* how many of a closed stream's last blocks hand their post-stage tasks out by ticket (measured: 2, 4, 6 end a 20-block stream
 * 36-38, 38-40, 38-41 us behind its last channel-IQ row -- what is left is the last block's own post stage) */
#define STREAM_DRAIN_BLOCKS 2u
/* ---- the bell ---- */
/* ---- the watcher: the second wave of the bell's workgroup.  It adds up the DDC waves' arrivals for the next block (a
 * shard per lane) and says so in ONE word (ddc_ready); it sees the post workgroups arrive and says, IN ORDER, which blocks
 * are finished -- to the DDC waves (post_ready: their ring rows are free again) and to the host (WrStreamCtl::done: the
 * block's ring slot is complete).  Nobody else polls a counter that arrivals land on. ---- */
__device__ __forceinline__ void stream_watch(const WrStreamArgs &S)
{
	const unsigned int lane = threadIdx.x & 63u;
	__builtin_amdgcn_s_setprio(3);
	const unsigned int units = S.k1 * S.groups;
	unsigned int known = 1, jd = 0, jp = 0;
	unsigned int df = 0;                             /* drain_from, once this wave has set it */
	unsigned int nlong = 0;                          /* blocks sent through in long runs (told to the host: WrStreamCtl::long_blocks) */
	bool closed = false;
	unsigned long long t_last = __builtin_amdgcn_s_memrealtime();
#ifdef STREAM_TL
	if ((threadIdx.x & 63u) == 0 && S.tl)
		S.tl[6999u * 8u + 0u] = t_last;                 /* the launch's first instructions */
#endif
	for (;;) {
		bool moved = false;
		/* a look at the doorbell's device-side copy: how many blocks are rung, and whether the stream is closed */
		auto look = [&]() __attribute__((always_inline)) {
			const unsigned int r = st_ld(&S.sdev->ready);
			if (r > known)
				known = r;
			if (st_ld(&S.sdev->stop)) {
				const unsigned int f = st_ld(&S.sdev->ready);
				if (f > known)
					known = f;
				closed = true;
				/* The drain: the last blocks' post stage is what the launch ends with (a block's post stage is one task per
				 * post workgroup and 20-26 us of memory round trips, and it trails the DDC by a block or two) while the DDC
				 * workgroups have run out of work.  From block max(known - 2, jd) on -- jd: not complete yet, so no post
				 * workgroup has begun it: they begin a block when `progress` says its channel IQ is complete, and this
				 * store is released before `progress` moves again -- tasks go by ticket to whoever asks, and the DDC
				 * workgroups ask (stream_post, `helper`). */
				const unsigned int from = known >= STREAM_DRAIN_BLOCKS ? known - STREAM_DRAIN_BLOCKS : 0u;
				df = (jd > from ? jd : from) + 1u;
				__hip_atomic_store(&S.sdev->drain_from, df, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
			}
		};
		if (!closed && (jd >= known || jp >= known))         /* (when it has caught up with what it knows of ...) */
			look();
		if (jd < known && jd < WR_STREAM_MAXJ) {
			unsigned int v = 0;
			if (lane < WR_STREAM_SHARDS)
				v = __hip_atomic_load(&S.sdev->ddc_done[jd][lane][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
			for (int o = 8; o >= 1; o >>= 1)
				v += __shfl_xor(v, o, 64);
			if (st_rfl(v) >= units) {
				{
					/* how block jd's post stage is cut (WrStreamDev::post_fine), said before anybody can begin it */
					/* (... and here, block jd complete but not said so yet: whether two further blocks are rung decides how it
					 * is cut -- and a close seen HERE still names jd as a block nobody has begun.  Looking only for the count
					 * and leaving the close to the look above lost the drain: with `known` up to date the watcher never "caught
					 * up" before the last block, the tickets were never handed out and a stream's last two blocks went one
					 * after the other on the post workgroups alone) */
					unsigned int fine = 1u;
					if (S.drain_run != S.post.run) {
						if (!closed)
							look();
						fine = (df && jd + 1u >= df) ? 1u : known >= jd + 3u ? 0u : 1u;
					}
					__hip_atomic_store(&S.sdev->post_fine[jd], fine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (!fine && lane == 0)
						st_st_sys(&S.ctl->long_blocks, ++nlong);
					asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				}
				++jd;
				__hip_atomic_store(&S.sdev->progress, ((unsigned long long)jp << 32) | jd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				moved = true;
#ifdef STREAM_TL
				if (lane == 0 && S.tl && jd <= 256u)
					S.tl[(7000u + jd - 1u) * 8u + 0u] = __builtin_amdgcn_s_memrealtime();
#endif
			}
		}
		/* (a block that went in short runs has more tasks: WrStreamDev::post_fine) */
		if (jp < jd && st_ld(&S.sdev->post_done[jp]) >= (st_ld(&S.sdev->post_fine[jp]) ? S.drain_ntiles : S.post.ntiles) * S.post.groups) {
			/* every task's stores of block jp are behind the release fence of the workgroup that ran it */
			++jp;
			__hip_atomic_store(&S.sdev->progress, ((unsigned long long)jp << 32) | jd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (lane == 0)
				st_st_sys(&S.ctl->done, jp);
			moved = true;
#ifdef STREAM_TL
			if (lane == 0 && S.tl && jp <= 256u)
				S.tl[(7000u + jp - 1u) * 8u + 1u] = __builtin_amdgcn_s_memrealtime();
#endif
		}
		if (closed && jp >= known)
			return;
		const unsigned long long now = __builtin_amdgcn_s_memrealtime();
		if (moved) {
			t_last = now;
		} else {
			if ((jd < known || jp < jd) && now - t_last > S.wait_ticks) {
				stream_fail(S);                          /* a block that is there and does not get done */
				return;
			}
			if (closed && st_ld_sys(&S.ctl->err))
				return;
			__builtin_amdgcn_s_sleep(4);
		}
	}
}

__device__ __forceinline__ void stream_bell(const WrStreamArgs &S)
{
	if (threadIdx.x >= 64u && threadIdx.x < 128u) {
		stream_watch(S);
		return;
	}
	if (threadIdx.x != 0)
		return;
	__builtin_amdgcn_s_setprio(3);
	unsigned int seen = 1;                              /* block 0: its descriptor came with the launch */
	__hip_atomic_store(&S.sdev->desc[0].cur, S.cur0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_store(&S.sdev->desc[0].audio_host, S.audio0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_store(&S.sdev->cur[1], S.cur0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    /* (before anything that says a second block is there) */
	unsigned long long t_last = __builtin_amdgcn_s_memrealtime();
	for (;;) {
		__hip_atomic_store(&S.sdev->beat, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
		                   __HIP_MEMORY_SCOPE_AGENT);
		/* stop first, then the count: the host writes them in the other order */
		const unsigned int s = st_ld_sys(&S.ctl->stop);
		unsigned int r = st_ld_sys(&S.ctl->ready);
		{
			/* (r06) ... and the doorbell in DEVICE memory: a block that came out of page-locked host memory is rung by a 4-byte
			 * copy queued behind the block's own on the upload stream (WrStreamDev::ready_up) -- in order with the data,
			 * without the host waiting for either */
			const unsigned int ru = st_ld(&S.sdev->ready_up);
			if (ru > r)
				r = ru;
		}
		if (r > WR_STREAM_MAXJ)
			r = WR_STREAM_MAXJ;
		if (r > seen) {
			for (unsigned int j = seen; j < r; ++j) {
				const unsigned long long c = __hip_atomic_load(&S.desc_host[j].cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
				const unsigned long long a = __hip_atomic_load(&S.desc_host[j].audio_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
				__hip_atomic_store(&S.sdev->desc[j].cur, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_store(&S.sdev->cur[j + 1u], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_store(&S.sdev->desc[j].audio_host, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__hip_atomic_store(&S.sdev->ready, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			seen = r;
			t_last = __builtin_amdgcn_s_memrealtime();
		}
		if (s || st_ld(&S.sdev->stop)) {                 /* the host's stop, or a wave's error */
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__hip_atomic_store(&S.sdev->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			return;
		}
		if (seen >= WR_STREAM_MAXJ || __builtin_amdgcn_s_memrealtime() - t_last > S.idle_ticks) {
			/* no room for another block, or nobody rang for too long: the launch ends with what it has.  (The host does
			 * not ring a stream it has left alone for a fraction of idle_ticks: it opens a new one.) */
			if (seen < WR_STREAM_MAXJ)
				st_st_sys(&S.ctl->self_closed, 1u);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__hip_atomic_store(&S.sdev->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			return;
		}
		__builtin_amdgcn_s_sleep(40);
	}
}

/* ---- the post stage, block by block ---- */
/* NSEG: the audio filter's taps / 64 (post_role): 1, or 2 / 4 for a filter of 128 / 256 taps -- the staged window and the
 * history in front of a block grow to 64 NSEG - 1 rows, everything else is the 64-tap launch's */
template <unsigned int PD2, unsigned int TS, unsigned int NSEG>
__device__ __forceinline__ void stream_post(const WrStreamArgs &S, const unsigned int p, v2f *lds, const bool helper)
{
	constexpr unsigned int D2 = PD2 ? PD2 : 1u;
	constexpr unsigned int NEED = (POST_TK - 1u) * D2 + WR_FIR_LENGTH * NSEG;
	wave_prio(3u);
	if (threadIdx.x >= POST_THREADS)
		return;
	const unsigned int wave = st_rfl(threadIdx.x >> 6);
	const unsigned int waves_per_wg = POST_THREADS / 64u;
#ifdef STREAM_TL
	if (threadIdx.x == 0 && S.tl && !helper)
		S.tl[(6000u + p) * 8u + 7u] = 12345ull;
#endif

	/* block 0's frames whose windows reach into the block before the stream: one wave per (lane group, frame), with the
	 * turns and LO values kept from back then -- k_tuner_ddc's block-boundary role, word for word */
	const unsigned int n_bnd = (S.kslow * S.groups + waves_per_wg - 1u) / waves_per_wg;
	if (!helper && p < n_bnd) {
		const unsigned long long c0 = S.cur0;
		ddc_body<WR_NCO_ROTATE, true, PD2>(S.is_u8 ? nullptr : (const float2 *)c0, S.is_u8 ? (const uchar2 *)c0 : nullptr,
		                                   (const float2 *)S.hist, (float2 *)S.hist_next, (size_t)S.nframes, (size_t)S.k1, S.d1,
		                                   S.slots, S.groups, S.phase, S.step, (const float2 *)S.hist_cs, S.flags, S.phase_next,
		                                   (float2 *)S.hist_cs_next, (const float2 *)S.hist_lo, (float2 *)S.hist_lo_next, S.taps1,
		                                   (const float4 *)S.rot, S.taps1u, S.tapsel, TS == 1u ? 1u : S.kmax, (float2 *)S.ring, S.table,
		                                   (const float2 *)S.hi_cs, (const float2 *)S.lo_cs, S.n_ddc, S.post, S.gmap0, S.gmap1, 0,
		                                   S.kslow, 0x40000000u, 0u, 0u, lds, DDC_ROLE_BOUNDARY);
		const unsigned int ub = p * waves_per_wg + wave;
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		if (ub / S.groups < S.kslow && (threadIdx.x & 63u) == 0u)
			__hip_atomic_fetch_add(&S.sdev->ddc_done[0][ub % WR_STREAM_SHARDS][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		wave_prio(3u);
		__syncthreads();                                 /* the role's LDS (tables, windows) is the post stage's from here on */
	}

	float *stage = (float *)lds;
	float *tile = stage + NEED * 64u;
	int *modes = (int *)(tile + POST_TK * 65u);
	unsigned int *sh = (unsigned int *)(modes + 64);    /* [0] go on, [1..2] the block's ring slot on the host */
	const unsigned int tasks = S.post.ntiles * S.post.groups;     /* tiles x lane groups; the state a block leaves behind is
	                                                                  written ONCE, behind the stream's last block (below) */
	unsigned int known = 1;                          /* block 0 is there from the start */
	bool closed = false;
	unsigned int j = 0;
	if (helper) {
		/* a DDC workgroup behind its last block and its share of the stream's state: the blocks whose post-stage tasks go
		 * by ticket, if there are any (WrStreamDev::drain_from) */
		if (threadIdx.x == 0)
			sh[6] = st_ld(&S.sdev->drain_from);
		__syncthreads();
		const unsigned int df = sh[6];
		if (!df)
			return;
		j = df - 1u;
	}
#ifdef STREAM_TL
	unsigned long long pt_wait = 0, pt_work = 0, pt_sync = 0, pt_n = 0;
#endif
	for (;; ++j) {
#ifdef STREAM_TL
		const unsigned long long pt0 = __builtin_amdgcn_s_memtime();
#endif
		if (threadIdx.x == 0) {
			bool ok = j < WR_STREAM_MAXJ && stream_wait_ready(S, j, known, closed);
			/* ... for the block's channel IQ (progress, low word) and -- the device audio array: block j stores into the one block
			 * j - 4 stored into (WrStreamArgs::audio_bufs), behind ALL of that block's stores -- for block j - 4's post stage
			 * (high word).  In a running stream of large blocks that is long done; with small blocks, whose post stages run up
			 * to four side by side (`rot` below), and in the drain, where tasks go by ticket to whoever asks, it is not a
			 * given (ADVICE r05).  ONE 8-byte load says both. */
			if (ok) {
				const unsigned int need_hi = j >= 4u ? j - 3u : 0u;
				const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
				unsigned int spins = 0;
				for (;;) {
					const unsigned long long pg = st_ld64(&S.sdev->progress);
					if ((unsigned int)pg >= j + 1u && (unsigned int)(pg >> 32) >= need_hi)
						break;
					if ((++spins & 63u) == 0u) {
						if (__builtin_amdgcn_s_memrealtime() - t0 > S.wait_ticks) {
							stream_fail(S);
							ok = false;
							break;
						}
						if (st_ld_sys(&S.ctl->err)) {
							ok = false;
							break;
						}
					}
					__builtin_amdgcn_s_sleep(20);
				}
			}
			unsigned long long ah = 0;
			unsigned int drain = helper ? 1u : 0u;
			if (ok) {
				ah = j ? st_ld64(&S.sdev->desc[j].audio_host) : S.audio0;
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
				if (!helper) {
					/* (read behind the acquire: a block from drain_from on is seen as such by every workgroup that begins it) */
					const unsigned int df = st_ld(&S.sdev->drain_from);
					drain = (df && j + 1u >= df) ? 1u : 0u;
				}
				sh[7] = (helper || drain) ? 1u : st_ld(&S.sdev->post_fine[j]);
			}
			sh[5] = drain;
			sh[0] = ok ? 1u : 0u;
			sh[1] = (unsigned int)ah;
			sh[2] = (unsigned int)(ah >> 32);
			sh[3] = known;
		}
		__syncthreads();
		const bool go = sh[0] != 0u;
		const unsigned long long ah = ((unsigned long long)sh[2] << 32) | sh[1];
		known = sh[3];
		if (!go)
			break;
		/* Block j's tiles.  The rows in front of the block -- the audio filter's 63 (64 NSEG - 1) rows of history, the
		 * demodulator's previous frame -- come from the tuner's state for block 0 and, for every later block, from the last
		 * 64 NSEG channel-IQ rows of the block before, which are still in the ring (WrPostArgs::chan_prev): a block's post
		 * stage waits for its own channel IQ and for nothing else, so the post workgroups need not move in step. */
		WrPostArgs A = S.post;
		A.chan_iq = S.ring + (size_t)(j % WR_STREAM_RING) * S.k1 * S.slots * 2u;
		A.chan_prev = j ? S.ring + (size_t)((j - 1u) % WR_STREAM_RING) * S.k1 * S.slots * 2u : nullptr;
		A.prev_iq = S.prev_iq[S.parity0];
		A.dem_hist = S.dem[S.parity0];
		A.audio_host = (float *)ah;
		A.audio = S.audio_bufs[j & 3u];
#ifdef STREAM_TL
		const unsigned long long pt1 = __builtin_amdgcn_s_memtime();
		if (threadIdx.x == 0 && S.tl && !helper && p < 4u && j < 256u)
			S.tl[(7300u + j) * 8u + p * 2u] = __builtin_amdgcn_s_memrealtime();
#endif
		const bool drain = sh[5] != 0u;
		if (sh[7] != 0u) {
			A.run = S.drain_run;
			A.ntiles = S.drain_ntiles;
		}
		const unsigned int tasks_j = A.ntiles * A.groups;
		unsigned int mine = 0;
		/* (r06) a block's tasks begin at another post workgroup every block: with fewer tasks than post workgroups (small
		 * blocks: BASELINE config 1 has 32 tasks a block) the post stages of consecutive blocks run side by side on
		 * different workgroups instead of queueing behind each other on the same ones -- a block's post stage is a
		 * chain of memory round trips, 18-20 us whatever its size */
		const unsigned int rot = (unsigned int)(((unsigned long long)j * tasks) % S.n_post);
		for (unsigned int t = p >= rot ? p - rot : p + S.n_post - rot;; t += S.n_post) {
			if (drain) {
				/* (the stream's last blocks: tasks by ticket, the idle DDC workgroups beside the post workgroups) */
				if (threadIdx.x == 0)
					sh[4] = __hip_atomic_fetch_add(&S.sdev->post_ticket[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__syncthreads();
				t = sh[4];
			}
			if (t >= tasks_j)
				break;
			post_role<D2, false, NSEG>(A, t % A.ntiles, t / A.ntiles, stage, tile, modes);
			__syncthreads();                             /* the next task's first phase rewrites `modes` and the stage */
			++mine;
		}
		/* (the barrier above: every wave's stores are issued; `sh` is free again) */
		if (threadIdx.x == 0 && mine) {
			if (ah)
				__builtin_amdgcn_fence(__ATOMIC_RELEASE, "");          /* the ring slot is the host's: system scope */
			else
				__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__hip_atomic_fetch_add(&S.sdev->post_done[j], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
#ifdef STREAM_TL
		if (threadIdx.x == 0 && S.tl && !helper && p < 4u && j < 256u)
			S.tl[(7300u + j) * 8u + p * 2u + 1u] = __builtin_amdgcn_s_memrealtime();
		if (threadIdx.x == 0) {
			const unsigned long long pt3 = __builtin_amdgcn_s_memtime();
			pt_wait += pt1 - pt0;
			pt_sync += pt3 - pt1;
			++pt_n;
		}
#endif
	}
#ifdef STREAM_TL
	if (threadIdx.x == 0 && S.tl && !helper) {
		S.tl[(6000u + p) * 8u + 0u] = pt_wait;
		S.tl[(6000u + p) * 8u + 1u] = pt_sync;
		S.tl[(6000u + p) * 8u + 2u] = pt_n;
	}
#endif
	/* The stream is closed and this workgroup has done its share of every block: what the LAST block leaves behind per
	 * lane group -- the last 63 (64 NSEG - 1) demodulator outputs, the last channel frame (post_role's state task) -- goes
	 * to the other ping-pong set, once: what a launch per block reads as its history, whatever the filter's length.
	 * (Every post workgroup has seen ddc_ready reach the last block: its rows are there.) */
	if (!helper && p < S.post.groups && known && known <= WR_STREAM_MAXJ) {
		const unsigned int jl = known - 1u;
		WrPostArgs A = S.post;
		A.chan_iq = S.ring + (size_t)(jl % WR_STREAM_RING) * S.k1 * S.slots * 2u;
		A.chan_prev = jl ? S.ring + (size_t)((jl - 1u) % WR_STREAM_RING) * S.k1 * S.slots * 2u : nullptr;
		A.prev_iq = S.prev_iq[S.parity0];
		A.dem_hist = S.dem[S.parity0];
		A.prev_next = const_cast<float *>(S.prev_iq[S.parity0 ^ 1]);
		A.dem_hist_next = S.dem[S.parity0 ^ 1];
		post_role<D2, false, NSEG>(A, A.ntiles, p, stage, tile, modes);
	}
}

/* ---- the DDC waves ----
 * TS: tap sets per lane group the instance provides for.  TS = 1: one channel filter per lane group (NG = 2: ONE for
 * both lane groups of a wave).  TS = WR_TAPSETS (NG = 1 only): up to that many distinct channel filters in a lane group,
 * S.kmax of them at most in this launch -- as k_tuner_ddc's lean loop, the window goes to LDS once per filter, tap *
 * sample, and a lane reads the copy made with ITS filter (WrGroupDev::tapsel): the same products, the same bits. */
template <unsigned int NG, unsigned int TS>
__device__ __forceinline__ void stream_ddc(const WrStreamArgs &S, v2f *lds)
{
	static_assert(TS == 1u || (TS == WR_TAPSETS && NG == 1u), "several channel filters: one lane group per wave");
	constexpr int NCO = WR_NCO_ROTATE;
	const unsigned int lane = threadIdx.x & 63u;
	const unsigned int wave = st_rfl(threadIdx.x >> 6);
	const unsigned int waves_per_wg = blockDim.x >> 6;
	const unsigned int wid = blockIdx.x * waves_per_wg + wave;
	wave_prio(3u);                                           /* the prologue's loads go out at once */
	rot_tables_to_lds(lds, (const float2 *)S.hi_cs, (const float2 *)S.lo_cs);
	const v2f *hi_l = lds, *lo_l = lds + WR_SPLIT_N;
	const unsigned int nset = TS == 1u ? 1u : S.kmax;        /* window copies per buffer, double buffered: [buffer][set][64] */
	v2f *win = lds + 2u * WR_SPLIT_N + wave * (128u * nset);
	const unsigned int k1s = S.k1, d1 = S.d1;
	const unsigned int nwaves = S.n_ddc * waves_per_wg;
	const unsigned int gsets = S.groups / NG;                /* sets of NG lane groups that share a wave */
	const unsigned int wpg = nwaves / gsets;                 /* >= 1: the launcher */
	const unsigned int gs = wid % gsets;
	const unsigned int iw = wid / gsets;
	unsigned int known = 1;                          /* block 0 is there from the start */
	bool closed = false;
	if (iw < wpg) {
		/* the wave's first output frame, as a frame of the STREAM: behind block 0's boundary frames */
		const unsigned long long q0 = (unsigned long long)S.kslow + iw;
		LeanRec<NG> R = lean_rec<NG>([&](unsigned int s) { return S.phase[s]; }, S.step, S.flags, (const float4 *)S.rot,
		                             (float2 *)S.ring, S.gmap0, S.gmap1, gs, lane, (unsigned int)(q0 * d1 - WR_HIST), wpg, d1);
		const LeanWin<TS> W = lean_win<TS>(S.taps1u, S.tapsel, R.g0, lane, nset, win);
		/* where the wave computes (block j, frame k of it) and where it fetches (two units ahead) */
		unsigned int j = 0, k = (unsigned int)q0;
		while (k >= k1s) {
			k -= k1s;
			++j;
		}
		unsigned int jf = j, kf = k;
		unsigned int jb = 0xFFFFFFFFu;                       /* block whose addresses are at hand */
		unsigned long long base_cur = 0, base_prev = 0;
		const bool u8 = S.is_u8 != 0u, ext = S.ext != 0u;
		/* The window of the unit two ahead is requested while a unit is computed -- but NEVER waited for a block that has
		 * not been submitted yet: a wave parked in such a wait would sit on units it already holds (and on the completion
		 * counts of the blocks it has left), and a block's audio would wait for the NEXT block to be rung.  A request
		 * for a block that is not there yet is simply not made; the wave works off what it holds, says what it has
		 * finished, and only then waits for the doorbell (the epochs of the loop below). */
		unsigned int ahead = 0;                           /* units whose windows are requested or in LDS, not yet computed */
		bool drain = false;                               /* a request could not be made: no further ones in this epoch (the
		                                                     two window registers take turns, unit by unit) */
		auto try_fetch = [&](float2 &dst) __attribute__((always_inline)) {
			if (drain)
				return;
			if (jf >= WR_STREAM_MAXJ) {
				drain = true;
				return;
			}
			if (jf >= known) {
				if (!closed) {
					const unsigned int r = st_ld(&S.sdev->ready);        /* one look, no wait */
					if (r > known)
						known = r;
					if (jf >= known && st_ld(&S.sdev->stop)) {
						const unsigned int f = st_ld(&S.sdev->ready);
						if (f > known)
							known = f;
						closed = true;
					}
				}
				if (jf >= known) {
					drain = true;
					return;
				}
			}
			if (jf != jb) {
				/* (both loads in flight together: one round trip) */
				if (jf) {
					const unsigned long long a0 = __hip_atomic_load(&S.sdev->cur[jf], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					const unsigned long long a1 = __hip_atomic_load(&S.sdev->cur[jf + 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					base_prev = ((unsigned long long)st_rfl((unsigned int)(a0 >> 32)) << 32) | st_rfl((unsigned int)a0);
					base_cur = ((unsigned long long)st_rfl((unsigned int)(a1 >> 32)) << 32) | st_rfl((unsigned int)a1);
				} else {
					base_prev = 0;                        /* (block 0's first frames are the boundary role's) */
					base_cur = S.cur0;
				}
				jb = jf;
			}
			/* window sample `lane` of frame kf of block jf: frame kf * d1 - 63 + lane of the block, or (the first
			 * ceil(63 / d1) frames of a block) of the block before -- never of block 0 here: q0 >= kslow */
			const long long n = (long long)kf * d1 - WR_HIST + lane;
			const unsigned long long base = (n >= 0) ? base_cur : base_prev;
			const unsigned long long idx = (n >= 0) ? (unsigned long long)n : (unsigned long long)((long long)S.nframes + n);
			/* (GLOBAL loads, said so: an address made from an integer is a generic pointer, a load through it a FLAT
			 * instruction -- which counts on the LDS counter too and returns out of order with the LDS reads, so that
			 * every wait for a window read in the tap loop became a wait for EVERYTHING: 12.3 k cycles per unit's taps
			 * instead of 8.4 k, r05) */
			if (ext) {
				/* (r06) agent-scope loads: they do not hit in an L2 that may still hold what the buffer held a few blocks ago -- a
				 * block the DMA engine wrote WHILE this launch was running (wr_tuner_submit_u8 out of page-locked host memory:
				 * WrStreamArgs::ext); a kernel's ordinary loads are only promised what was there when it started */
				if (u8) {
					const unsigned short b2 = __hip_atomic_load((const __attribute__((address_space(1))) unsigned short *)base + idx,
					                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					dst = make_float2(__builtin_bit_cast(float, (unsigned int)b2), 0.0f);
				} else {
					const unsigned long long x2 = __hip_atomic_load((const __attribute__((address_space(1))) unsigned long long *)base + idx,
					                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					dst = make_float2(__builtin_bit_cast(float, (unsigned int)x2), __builtin_bit_cast(float, (unsigned int)(x2 >> 32)));
				}
			} else if (u8) {
				const unsigned short b2 = ((const __attribute__((address_space(1))) unsigned short *)base)[idx];
				dst = make_float2(__builtin_bit_cast(float, (unsigned int)b2), 0.0f);
			} else {
				const v2f x2 = ((const __attribute__((address_space(1))) v2f *)base)[idx];
				dst = make_float2(x2.x, x2.y);
			}
			++ahead;
			kf += wpg;
			while (kf >= k1s) {
				kf -= k1s;
				++jf;
			}
		};
		unsigned int cnt = 0, pend_j = 0, pend_cnt = 0;   /* lane-group units done in block j / to be signalled for pend_j */
		unsigned int jring = 0xFFFFFFFFu;                 /* block whose ring rows are known to be free */
		/* everything this wave has finished and not said yet: the block it left last (all of its stores are waited for) */
		auto tell = [&]() __attribute__((always_inline)) {
			if (pend_cnt) {
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				if (lane == 0)
					__hip_atomic_fetch_add(&S.sdev->ddc_done[pend_j][wid % WR_STREAM_SHARDS][0], pend_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				pend_cnt = 0;
			}
		};
		static_assert(ROT_SEG == WR_FIR_LENGTH, "one recurrence over the whole window");
		float2 xa = make_float2(0.0f, 0.0f), xb = xa;
		/* one unit from LDS buffer b; `xo` holds the NEXT unit's window sample (on its way or landed) if ahead >= 2 */
		unsigned long long tl_taps = 0, tl_rest = 0, tl_wait = 0, tl_units = 0, tl_ring = 0, tl_ringn = 0, tl_epochs = 0;
#ifdef STREAM_TL
		const bool tl_on = S.tl != nullptr;
#else
		constexpr bool tl_on = false;                     /* (s_memtime is a scalar memory instruction: even behind a branch it
		                                                     makes every LDS wait of the tap loop a wait for everything) */
#endif
		unsigned int lead = 0;                            /* blocks this wave is ahead of the slowest one (as of its entry into block j) */
		auto unit = [&](float2 &xo, const int b) __attribute__((always_inline)) {
			const unsigned long long tl0 = tl_on ? __builtin_amdgcn_s_memtime() : 0ull;
			if (j != jring) {
				/* Entering a block.  (1) WHO GOES FIRST on the SIMD: the issue arbiter goes by priority, then age -- at
				 * equal priority the oldest waves of a SIMD take every VALU slot and the youngest fall blocks behind, until
				 * the old ones run into the ring's end and wait while the stragglers work alone at a third of the issue
				 * rate (r05, measured: every wave 20 us per block in that wait, 57 % of the issue rate).  So a wave's
				 * priority follows its LEAD over the slowest wave, in blocks: whoever is behind goes first, as k_tuner_ddc
				 * does within a launch.
				 * (2) the ring rows of block j were block j - RING's: its post stage must be through with them, and so must
				 * the post stage of block j - RING + 1, which reads that block's last rows as its history.  (Before the
				 * wave waits for anybody it says what it has finished: that post stage may be waiting for THIS wave.) */
				const unsigned long long pg = __hip_atomic_load(&S.sdev->progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				const unsigned int dr = st_rfl((unsigned int)pg), pr = st_rfl((unsigned int)(pg >> 32));
				lead = j > dr ? j - dr : 0u;
				if (j + 1u >= WR_STREAM_RING && pr < j - WR_STREAM_RING + 2u) {
					const unsigned long long tw0 = tl_on ? __builtin_amdgcn_s_memtime() : 0ull;
					tell();
					if (!stream_wait_count(S, (const unsigned int *)&S.sdev->progress + 1, j - WR_STREAM_RING + 2u)) {
						known = j;                       /* an error somewhere: this unit is the wave's last */
						closed = true;
					}
					if (tl_on) {
						tl_ring += __builtin_amdgcn_s_memtime() - tw0;
						++tl_ringn;
#ifdef STREAM_TL
						if (lane == 0 && S.tl && (wid % 1000u) == 0u && j < 256u)
							S.tl[(7600u + j) * 8u + 4u + wid / 1000u] = __builtin_amdgcn_s_memrealtime();
#endif
					}
				}
				jring = j;
			}
			{
				/* ... and within a block it falls as the wave gets through it (quarters of the block's frames) */
				wave_prio(lead <= 1u ? 2u : lead <= 3u ? 1u : 0u);
			}
			const AccN<NG> acc = rotate_unit<NG>(W.w4[b], R, S.table, hi_l, lo_l);
			const unsigned long long tl1 = tl_on ? __builtin_amdgcn_s_memtime() : 0ull;
			/* the next unit's window (requested two units ago), if there is a next unit ... */
			if (ahead >= 2u)
				W.to_lds(xo, b ^ 1, u8);
			unsigned long long tl2 = 0;
			if (tl_on) {
				asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
				tl2 = __builtin_amdgcn_s_memtime();
			}
			/* ... the completion of the block this wave left a unit ago: its last store went out a whole unit back, and
			 * the only vector memory operations since are window loads as old -- the wait in tell() waits for nothing */
			tell();
			/* ... this unit's result, the request after next */
			const size_t row = (size_t)(j % WR_STREAM_RING) * k1s + k;
#pragma unroll
			for (unsigned int c = 0; c < NG; ++c) {
				if (R.fl[c] & PHASE_FLAG_ACTIVE) {
					union { v2f f; unsigned long long u; } cv;
					cv.f = acc.v[c];
					__hip_atomic_store((unsigned long long *)&R.out[c][row * S.slots], cv.u, __ATOMIC_RELAXED,
					                   __HIP_MEMORY_SCOPE_AGENT);             /* write-through: see ddc_body */
				}
				R.Pk[c] += R.dP[c];
			}
			--ahead;
			cnt += NG;
			k += wpg;
			if (k >= k1s) {
				pend_j = j;
				pend_cnt = cnt;
				cnt = 0;
				do {
					k -= k1s;
					++j;
				} while (k >= k1s);
			}
			try_fetch(xo);
			if (tl_on) {
				const unsigned long long tl3 = __builtin_amdgcn_s_memtime();
				tl_taps += tl1 - tl0;
				tl_wait += tl2 - tl1;
				tl_rest += tl3 - tl2;
				++tl_units;
			}
		};
		/* Epochs.  One begins with nothing requested: the wave waits for the block its next unit lies in (having said
		 * everything it has finished), requests up to three windows and works until it holds no more -- in a stream that
		 * the host keeps ahead of, that is the end of the stream. */
		for (;;) {
			if (j >= WR_STREAM_MAXJ || !stream_wait_ready(S, j, known, closed))
				break;
			drain = false;
			++tl_epochs;
			try_fetch(xa);                                /* unit 0 (there: the wait above) */
			try_fetch(xb);                                /* unit 1 */
			W.to_lds(xa, 0, u8);
			try_fetch(xa);                                /* unit 2 */
			wave_prio(2u);                                /* (set again at every block the wave enters) */
			while (ahead) {
				unit(xb, 0);
				if (!ahead)
					break;
				unit(xa, 1);
			}
			wave_prio(3u);
			tell();
		}
		if (tl_on && lane == 0 && S.tl) {
			S.tl[wid * 8u + 0u] = tl_taps;
			S.tl[wid * 8u + 1u] = tl_wait;
			S.tl[wid * 8u + 2u] = tl_rest;
			S.tl[wid * 8u + 3u] = tl_units;
			S.tl[wid * 8u + 4u] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     /* HW_ID */
			S.tl[wid * 8u + 5u] = __builtin_amdgcn_s_getreg((31 << 11) | 20);    /* XCC_ID */
			S.tl[wid * 8u + 6u] = tl_ring;
			S.tl[wid * 8u + 7u] = (tl_ringn << 32) | tl_epochs;
		}
		/* what is left to signal: the part of the block the stream ended in (if an error ended it there) */
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		if (lane == 0) {
			if (pend_cnt)
				__hip_atomic_fetch_add(&S.sdev->ddc_done[pend_j][wid % WR_STREAM_SHARDS][0], pend_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (cnt && j < WR_STREAM_MAXJ)
				__hip_atomic_fetch_add(&S.sdev->ddc_done[j][wid % WR_STREAM_SHARDS][0], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	wave_prio(0u);
	/* the stream is closed (a wave leaves its loop for no other reason; the waves left over wait for it here): `known`
	 * blocks went through.  The state every channel has behind them goes to the OTHER state set, as k_tuner_ddc's
	 * end-of-block roll does for one block -- the phase nframes * known steps on (downconverter.cxx:103), the turns and
	 * LO values of the last 63 frames (whatever setIF does before the next block) -- by all DDC waves together. */
	(void)stream_wait_ready(S, 0xFFFFFFFEu, known, closed);
	const unsigned long long total = S.nframes * known;           /* frames of the stream */
	const unsigned int gtid = wid * 64u + lane, gsz = nwaves * 64u;
	const float *table = S.table;
	for (unsigned int s = gtid; s < S.slots; s += gsz) {
		const bool act = (S.flags[s] & PHASE_FLAG_ACTIVE) != 0;
		S.phase_next[s] = act ? S.phase[s] + (unsigned int)total * S.step[s] : S.phase[s];
	}
	for (unsigned int e = gtid; e < WR_HIST * S.slots; e += gsz) {
		const unsigned int r = e / S.slots, s = e - r * S.slots;
		const unsigned long long f = total + r;          /* frame index in [63 frames of history | stream]: >= 63 */
		v2f cs = {0.0f, 0.0f}, lo = {0.0f, 0.0f};
		if (S.flags[s] & PHASE_FLAG_ACTIVE) {
			lo = nco<NCO>(S.phase[s] + (unsigned int)(f - WR_HIST) * S.step[s], table, hi_l, lo_l);
			cs = rot_into(S.phase[s], S.step[s], (unsigned int)(f - (WR_HIST - 1)), table);
		}
		((float2 *)S.hist_lo_next)[e] = make_float2(lo.x, lo.y);
		((float2 *)S.hist_cs_next)[e] = make_float2(cs.x, cs.y);
	}
	if (wid == 0 && known) {
		/* the tuner's next input history: the last 63 frames of the last block */
		const unsigned long long c = known > 1u ? st_ld64(&S.sdev->desc[known - 1u].cur) : S.cur0;
		if (lane < WR_HIST) {
			const size_t n = (size_t)(S.nframes - WR_HIST + lane);
			float2 v;
			if (S.ext && S.is_u8) {
				/* (a block the DMA engine wrote while the launch ran: not through a cache that may know an older one) */
				const unsigned int b = __hip_atomic_load((const unsigned short *)c + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				v = make_float2(((float)(b & 255u) - 128.0f) / 128.0f, ((float)(b >> 8) - 128.0f) / 128.0f);
			} else if (S.ext) {
				const unsigned long long x = __hip_atomic_load((const unsigned long long *)c + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				v = make_float2(__builtin_bit_cast(float, (unsigned int)x), __builtin_bit_cast(float, (unsigned int)(x >> 32)));
			} else {
				v = input_frame(S.is_u8 ? nullptr : (const float2 *)c, S.is_u8 ? (const uchar2 *)c : nullptr, n);
			}
			((float2 *)S.hist_next)[lane] = v;
		}
		if (lane == 0)
			st_st_sys(&S.ctl->final_blocks, known);
	}
}

template <unsigned int PD2, unsigned int NG, unsigned int TS, unsigned int NSEG>
__global__ void __launch_bounds__(DDC_ROTATE_WAVES * 64u) __attribute__((amdgpu_waves_per_eu(DDC_NG2_WAVES_PER_EU)))
k_tuner_stream(const WrStreamArgs S)
{
	extern __shared__ v2f lds[];
	if (blockIdx.x >= S.n_ddc + S.n_post) {
		stream_bell(S);
		return;
	}
	const bool ddc = blockIdx.x < S.n_ddc;
	if (ddc) {
		stream_ddc<NG, TS>(S, lds);
		__syncthreads();                                    /* every wave is behind its last block and the state roll: the
		                                                       workgroup's LDS is free, and so is the workgroup (stream_post) */
	}
	stream_post<PD2, TS, NSEG>(S, ddc ? blockIdx.x : blockIdx.x - S.n_ddc, lds, ddc);
}

/* (which instance a launch takes, its LDS and its roles: wrp_stream_plan, wrp_stream_roles; its post tiling:
 * wrp_post_tiling_stream -- wr_plan.h) */

/* calls f with the run-time nseg as a compile-time constant; a length the launch is not built for: hipErrorInvalidValue */
template <unsigned int PD2, class F>
static hipError_t with_stream_nseg(unsigned int nseg, F &&f)
{
	if (nseg == 1u)
		return f(std::integral_constant<unsigned int, 1u>());
	if (nseg == 2u)
		return f(std::integral_constant<unsigned int, 2u>());
	if constexpr (PD2 <= STREAM_NSEG4_MAX_D2)
		if (nseg == 4u)
			return f(std::integral_constant<unsigned int, 4u>());
	return hipErrorInvalidValue;
}

/* calls f(StreamInst<PD2, NG, TS, NSEG>()) for the instance the plan `P` of a launch with audio decimation `d2` and `nseg` names */
template <unsigned int PD2_, unsigned int NG_, unsigned int TS_, unsigned int NSEG_> struct StreamInst {
	static constexpr unsigned int PD2 = PD2_, NG = NG_, TS = TS_, NSEG = NSEG_;
};
template <class F>
static hipError_t with_stream_instance(const WrStreamPlan &P, unsigned int d2, unsigned int nseg, F &&f)
{
	return with_post_d2(d2, [&](auto D2) {
		constexpr unsigned int PD2 = decltype(D2)::value;
		return with_stream_nseg<PD2>(nseg, [&](auto NS) {
			constexpr unsigned int NSEG = decltype(NS)::value;
			return P.ts != 1u ? f(StreamInst<PD2, 1, WR_TAPSETS, NSEG>())
			       : P.ng == 1u ? f(StreamInst<PD2, 1, 1, NSEG>())
			                    : f(StreamInst<PD2, 2, 1, NSEG>());
		});
	});
}

/* An instance's dynamic LDS above 64 KB must be allowed once per device (allow_lds remembers that it has been): the MOST
 * the instance can ask for -- TS window copies per buffer -- not what this launch asks for.  With the current request a
 * tuner whose lane groups came to mix more channel filters later (kmax up, more window copies) kept the limit of its first
 * launch.  The 64-tap instances stay under 64 KB whatever kmax and never get here. */
template <unsigned int PD2, unsigned int NG, unsigned int TS, unsigned int NSEG>
static hipError_t stream_allow_lds(size_t lds)
{
	static bool attr_done[WR_MAX_DEVICES];
	if (lds <= 64 * 1024)
		return hipSuccess;
	return allow_lds((const void *)k_tuner_stream<PD2, NG, TS, NSEG>, stream_lds_bytes(PD2, TS, NSEG), attr_done);
}

/* How many workgroups of the streaming launch a device holds at once, split into roles (wrp_stream_roles), by the
 * occupancy query for the instance the launch takes */
hipError_t wrk_stream_geometry(unsigned int d2, unsigned int groups, unsigned int kmax, bool one_filter, unsigned int nseg,
                               int num_cus, unsigned int *n_ddc, unsigned int *n_post)
{
	*n_ddc = *n_post = 0;
	const WrStreamPlan P = wrp_stream_plan(d2, groups, kmax, one_filter, nseg);
	if (!P.ok)
		return hipSuccess;
	int per_cu = 0;
	hipError_t e = with_stream_instance(P, d2, nseg, [&](auto I) {
		using K = decltype(I);
		hipError_t e2 = stream_allow_lds<K::PD2, K::NG, K::TS, K::NSEG>(P.lds);
		if (e2 != hipSuccess)
			return e2;
		return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_tuner_stream<K::PD2, K::NG, K::TS, K::NSEG>,
		                                                    (int)(DDC_ROTATE_WAVES * 64u), P.lds);
	});
	if (e != hipSuccess)
		return e;
	const WrStreamRoles R = wrp_stream_roles(per_cu, num_cus);
	*n_ddc = R.n_ddc;
	*n_post = R.n_post;
	return hipSuccess;
}

/* `A.post` comes from wrk_post_args for ONE block of the stream; its tiling is redone here for the post workgroups
 * the launch keeps resident */
hipError_t wrk_tuner_stream(hipStream_t st, const WrStreamArgs &A0, void *ev_start, void *ev_stop)
{
	WrStreamArgs A = A0;
	if (!A.n_ddc || !A.n_post || !A.k1)
		return hipErrorInvalidValue;
	const WrStreamPlan P = wrp_stream_plan(A.post.d2, A.groups, A.kmax, A.one_filter != 0u, A.post.nseg);
	if (!P.ok || (size_t)A.n_ddc * DDC_ROTATE_WAVES < A.groups / P.ng)
		return hipErrorInvalidValue;
	/* (a block shorter than the audio filter has no L2 - 1 rows of history for the block behind it: wrc_stream_open) */
	if (A.k1 < WR_FIR_LENGTH * A.post.nseg)
		return hipErrorInvalidValue;
	const WrStreamTiling T = wrp_post_tiling_stream(A.post.tiles, A.post.groups, A.n_post);
	A.post.run = T.run;
	A.post.ntiles = T.ntiles;
	A.drain_run = T.drain_run;
	A.drain_ntiles = T.drain_ntiles;
	return with_stream_instance(P, A.post.d2, A.post.nseg, [&](auto I) {
		using K = decltype(I);
		hipError_t e = stream_allow_lds<K::PD2, K::NG, K::TS, K::NSEG>(P.lds);
		if (e != hipSuccess)
			return e;
		launch_stamped(k_tuner_stream<K::PD2, K::NG, K::TS, K::NSEG>, dim3(A.n_ddc + A.n_post + 1u), dim3(DDC_ROTATE_WAVES * 64u), P.lds, st,
		               ev_start, ev_stop, A);
		return hipGetLastError();
	});
}
