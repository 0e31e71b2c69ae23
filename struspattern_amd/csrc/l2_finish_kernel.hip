// Finishing passes of a device batch (l2_finish.h): count, offsets, place; for the canonical order a sort before place.
#include <hip/hip_runtime.h>
#include "l2_device.h"
#include "doc_passes.h"
#include "l2_finish.h"

using namespace spa;

namespace {

// The raw blocks of document d: results [first, first+count), items [itemFirst, itemFirst+itemCount).  False when the
// document counts as empty: it failed, its range does not fit the buffer (the two conditions of copyOutBatch), or it has no results.
__device__ __forceinline__ bool docBlocks( const FinishParams& P, u32 d, u64& first, u64& count, u64& itemFirst, u64& itemCount)
{
	const u64 devResults = P.nofResults, devItems = P.nofItems;
	first = P.docRange[ 2*(u64)d]; count = P.docRange[ 2*(u64)d+1];
	itemFirst = 0; itemCount = 0;
	if (P.docStatus[ d] != 0 || count == 0 || count > devResults || first > devResults - count) return false;
	// one item block per document, item_begin = block start + item counts before (l2_finish.h)
	const u32* r0 = P.results + 9*first;
	const u32* rl = P.results + 9*(first + count - 1);
	itemFirst = r0[ 7];
	itemCount = (u32)(rl[ 7] + rl[ 8] - r0[ 7]);
	return itemCount <= devItems && itemFirst <= devItems - itemCount;
}

// ---- pass A without `exclusive`: every result of a good document survives; a thread per document
__device__ void countDocuments( const FinishParams& P)
{
	for (u64 d = (u64)blockIdx.x*blockDim.x + threadIdx.x; d < P.ndocs; d += (u64)gridDim.x*blockDim.x)
	{
		u64 first, count, itemFirst, itemCount;
		const bool ok = docBlocks( P, (u32)d, first, count, itemFirst, itemCount);
		P.kept[ 2*d] = ok ? (u32)count : 0u;
		P.kept[ 2*d+1] = ok ? (u32)itemCount : 0u;
	}
}

// ---- pass A with `exclusive`: a wave per document marks the covered results (src/patternMatcher.cpp:192-246), a lane
// per result ai walking ni = ai, ai+1, .. to the reference's break condition.  The marks are idempotent and depend on
// the two records only, so all ai at once give the flags of the sequential loop.
__device__ void markDocuments( const FinishParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		u64 first, count, itemFirst, itemCount;
		const bool ok = uni( docBlocks( P, doc, first, count, itemFirst, itemCount) ? 1u : 0u) != 0;
		u32 kept = 0, keptItems = 0;
		if (ok)
		{
			first = uni64( first);
			const u32 n = uni( (u32)count);
			const u32* R = P.results + 9*first;
			uint8_t* C = P.covered + first;
			for (u32 base=0; base<n; base+=64)
			{
				const u32 ai = base + LANE;
				if (ai >= n) continue;
				const u32* r = R + 9*(u64)ai;
				const u32 rseg = r[ 3], rpos = r[ 4], rendseg = r[ 5], rend = r[ 6];
				bool cov = false;
				for (u32 ni=ai; ni<n; ++ni)
				{
					const u32* f = R + 9*(u64)ni;
					const u32 fseg = f[ 3], fpos = f[ 4], fendseg = f[ 5], fend = f[ 6];
					if (fseg > rendseg || fpos >= rend + P.maxResultSize) break;
					const bool differ = (fendseg != rendseg || fend != rend || fseg != rseg || fpos != rpos);
					if (fseg <= rseg && fpos <= rpos && fendseg >= rendseg && fend >= rend && differ) cov = true;
					if (fseg >= rseg && fpos >= rpos && fendseg <= rendseg && fend <= rend && differ) C[ ni] = 1;
				}
				if (cov) C[ ai] = 1;
			}
			__threadfence();		// the flags of the other lanes, before they are counted
			for (u32 base=0; base<n; base+=64)
			{
				const u32 ri = base + LANE;
				const bool keep = ri < n && C[ ri] == 0;
				const u32 ic = keep ? R[ 9*(u64)ri + 8] : 0u;
				kept += (u32)__popcll( __ballot( keep));
				keptItems += uni( (u32)__shfl( (int)waveScanAdd( ic), 63));
			}
		}
		if (LANE == 0) { P.kept[ 2*(u64)doc] = kept; P.kept[ 2*(u64)doc+1] = keptItems; }
	}
}

// ---- pass B: the offsets of the kept results and of the kept items of every document, in one trip (doc_passes.h).
// The sums inside a tile are 32 bit: the kept records are a subset of the batch's, and its buffers hold at most 2^32-1.
__device__ void scanDocuments( const FinishParams& P)
{
	const DocSums<2> total = scanDocumentCounts<u32, 2>( P.ndocs,
		[&]( u64 d) { const uint2 v = ((const uint2*)P.kept)[ d]; return DocCounts<2>{{ v.x, v.y}}; },
		[&]( u64 d, const DocCounts<2>&, const DocSums<2>& at) { P.docResultOffsets[ d] = at.v[ 0]; P.docItemOffsets[ d] = at.v[ 1]; });
	if (threadIdx.x == 0)
	{
		P.docResultOffsets[ P.ndocs] = total.v[ 0]; P.docItemOffsets[ P.ndocs] = total.v[ 1];
		P.totals[ 0] = total.v[ 0]; P.totals[ 1] = total.v[ 1];
	}
}

// ---- pass C
// The word of a result record that is its item_begin gets `delta` added; r = (index of v.x in the block) mod 9
__device__ __forceinline__ void rebase( u32x4& v, u32 r, u32 delta)
{
	if (r == 7) v.x += delta; else if (r == 6) v.y += delta; else if (r == 5) v.z += delta; else if (r == 4) v.w += delta;
}
__device__ __forceinline__ u32 mod9( u32 r) { return r >= 9 ? r - 9 : r; }

// Streaming copy of n words by one wave: 16-byte stores to the aligned part of dst, 16-byte loads from wherever that
// leaves src (blocks are 4-byte aligned only), up to 3 single words at the head and at the tail.  REBASE: the block is a
// run of result records starting with a whole one, and word 7 of every 9 gets `delta` added.
template <bool REBASE>
__device__ __forceinline__ void copyWords( u32* dst, const u32* src, u64 n, u32 delta)
{
	u32 head = (4u - (u32)(((uintptr_t)dst >> 2) & 3u)) & 3u;
	if (head > n) head = (u32)n;
	if (LANE < head) dst[ LANE] = src[ LANE];		// (words 0..2 of a record: nothing to rebase)
	const u64 nvec = (n - head) >> 2;
	const u32x4u* s = (const u32x4u*)(src + head);
	u32x4* t = (u32x4*)(dst + head);
	u32 r = (head + 4*LANE) % 9;			// 64 vectors on: 256 words = 4 mod 9
	u64 v = LANE;
	for (; v + 192 < nvec; v += 256)
	{
		u32x4 a = s[ v], b = s[ v+64], c = s[ v+128], d = s[ v+192];
		if (REBASE)
		{
			const u32 r1 = mod9( r + 4), r2 = mod9( r1 + 4), r3 = mod9( r2 + 4);
			rebase( a, r, delta); rebase( b, r1, delta); rebase( c, r2, delta); rebase( d, r3, delta);
			r = mod9( r3 + 4);
		}
		t[ v] = a; t[ v+64] = b; t[ v+128] = c; t[ v+192] = d;
	}
	for (; v < nvec; v += 64)
	{
		u32x4 a = s[ v];
		if (REBASE) { rebase( a, r, delta); r = mod9( r + 4); }
		t[ v] = a;
	}
	const u64 done = head + 4*nvec;
	if (LANE < (u32)(n - done))
	{
		u32 x = src[ done + LANE];
		if (REBASE && (done + LANE) % 9 == 7) x += delta;
		dst[ done + LANE] = x;
	}
}

// A surviving result by its lane: the record r, result `src` of the batch, becomes result `mine` of the output, and its
// ic items from item ib on the items from myItems on; with formats, their format words go with them.
__device__ __forceinline__ void placeResult( const FinishParams& P, const u32* r, u64 src, u64 mine, u32 ib, u32 ic, u64 myItems)
{
	u32* o = P.outResults + 9*mine;
	for (u32 k=0; k<7; ++k) o[ k] = r[ k];
	o[ 7] = (u32)myItems; o[ 8] = ic;
	const u32* si = P.items + 7*(u64)ib;
	u32* di = P.outItems + 7*myItems;
	for (u32 k=0; k<7*ic; ++k) di[ k] = si[ k];
	if (P.withFormats)
	{
		P.outResultFormat[ mine] = P.resultFormat[ src];
		for (u32 k=0; k<2*ic; ++k) P.outItemFormat[ 2*myItems + k] = P.itemFormat[ 2*(u64)ib + k];
	}
}

__device__ void placeDocuments( const FinishParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 rp = uni64( P.docResultOffsets[ doc]), nk = uni64( P.docResultOffsets[ doc+1]) - rp;
		const u64 ip = uni64( P.docItemOffsets[ doc]), nki = uni64( P.docItemOffsets[ doc+1]) - ip;
		if (nk == 0) continue;
		if (rp + nk > P.nofResults || ip + nki > P.nofItems) continue;	// (the survivors are a subset: what the host sized holds them)
		const u64 first = uni64( P.docRange[ 2*(u64)doc]);
		const u32* R = P.results + 9*first;
		if (!P.exclusive)
		{
			// every result survives: two blocks move as they are, item_begin rebased by the document's constant
			const u64 itemFirst = uni( R[ 7]);
			copyWords<true>( P.outResults + 9*rp, R, 9*nk, (u32)ip - (u32)itemFirst);
			copyWords<false>( P.outItems + 7*ip, P.items + 7*itemFirst, 7*nki, 0);
			if (P.withFormats)
			{
				copyWords<false>( P.outResultFormat + rp, P.resultFormat + first, nk, 0);
				copyWords<false>( P.outItemFormat + 2*ip, P.itemFormat + 2*itemFirst, 2*nki, 0);
			}
		}
		else
		{
			// a lane per result: the survivors keep their order, rank by ballot, items by prefix sum of their counts
			const u32 n = uni( (u32)P.docRange[ 2*(u64)doc+1]);
			const uint8_t* C = P.covered + first;
			u64 rat = rp, iat = ip;
			for (u32 base=0; base<n; base+=64)
			{
				const u32 ri = base + LANE;
				const bool keep = ri < n && C[ ri] == 0;
				const u32* r = R + 9*(u64)ri;
				const u32 ib = keep ? r[ 7] : 0u, ic = keep ? r[ 8] : 0u;
				const u64 mask = __ballot( keep);
				const u32 iincl = waveScanAdd( ic);
				if (keep)
				{
					const u64 mine = rat + (u32)__popcll( mask & ((1ull << LANE) - 1ull));
					const u64 myItems = iat + (iincl - ic);
					placeResult( P, r, first + ri, mine, ib, ic, myItems);
				}
				rat += (u32)__popcll( mask);
				iat += uni( (u32)__shfl( (int)iincl, 63));
			}
		}
	}
}

// ---- canonical order (l2_finish.h): between passes B and C a workgroup per document sorts {key64 = ordpos << 32 | ordend,
// index in the raw block} entries of the survivors; pass C then places through the sorted indices.
enum { SORT_THREADS = 512, SORT_WAVES = SORT_THREADS/64, MERGE_RUN = 16 };	// MERGE_RUN divides the tile: a run of outputs never crosses a pair of runs
const u32 NO_ENTRY = 0xFFFFFFFFu;		// index of the padding entries (key all ones): they sort behind every result

struct SortDoc
{
	const FinishParams& P;
	const u32* R;		// the raw result block
	u64 first;		// its first result
	u32 n;			// results in it
};

// T(a) < T(b) for two results with the same key64: the rest of the tuple from the records, then their items
__device__ bool tieLess( const SortDoc& D, u32 ia, u32 ib)
{
	const FinishParams& P = D.P;
	const u32* a = D.R + 9*(u64)ia;
	const u32* b = D.R + 9*(u64)ib;
	for (u32 w=3; w<=6; ++w) if (a[ w] != b[ w]) return a[ w] < b[ w];
	if (a[ 0] != b[ 0]) return a[ 0] < b[ 0];
	const u32 ic = a[ 8];
	if (ic != b[ 8]) return ic < b[ 8];
	if (P.withFormats)
	{
		const u32 fa = P.resultFormat[ D.first + ia], fb = P.resultFormat[ D.first + ib];
		if (fa != fb) return fa < fb;
	}
	const u64 ab = a[ 7], bb = b[ 7];
	if (ab + ic <= P.nofItems && bb + ic <= P.nofItems)
	{
		const u32* x = P.items + 7*ab;
		const u32* y = P.items + 7*bb;
		for (u32 w=0; w<7*ic; ++w) if (x[ w] != y[ w]) return x[ w] < y[ w];
		if (P.withFormats)
		{
			x = P.itemFormat + 2*ab; y = P.itemFormat + 2*bb;
			for (u32 w=0; w<2*ic; ++w) if (x[ w] != y[ w]) return x[ w] < y[ w];
		}
	}
	return ia < ib;		// equal tuples: the finished records are the same bytes in either order
}

__device__ __forceinline__ bool entryLess( const SortDoc& D, u64 ka, u32 ia, u64 kb, u32 ib)
{
	if (ka != kb) return ka < kb;
	if (ia == ib) return false;
	if (ia >= D.n || ib >= D.n) return ia < ib;	// padding
	return tieLess( D, ia, ib);
}

// the stages j = jfirst, jfirst/2, .. 1 (jfirst <= 32) of the bitonic level k on 64 consecutive entries, one per lane,
// element i of the sequence in this lane: the partner comes over the cross-lane network, nothing goes through LDS
__device__ __forceinline__ void waveStages( const SortDoc& D, u64& key, u32& idx, u32 i, u32 k, u32 jfirst)
{
	for (u32 j=jfirst; j>=1; j>>=1)
	{
		const u32 phi = (u32)__shfl_xor( (int)(u32)(key >> 32), (int)j), plo = (u32)__shfl_xor( (int)(u32)key, (int)j);
		const u32 pidx = (u32)__shfl_xor( (int)idx, (int)j);
		const u64 pkey = ((u64)phi << 32) | plo;
		const bool wantMin = ((i & j) == 0) == ((i & k) == 0);
		const bool mineLess = entryLess( D, key, idx, pkey, pidx);
		if (wantMin != mineLess) { key = pkey; idx = pidx; }
	}
}

__device__ __forceinline__ u32 sortLevels( u64 nk)	// merge passes of a document with nk survivors: the buffer its order ends in is levels & 1
{
	u32 l = 0;
	for (u64 w=FINISH_SORT_TILE; w<nk; w<<=1) ++l;
	return l;
}

__device__ void sortDocuments( const FinishParams& P)
{
	__shared__ u64 K[ FINISH_SORT_TILE];
	__shared__ u32 I[ FINISH_SORT_TILE];
	__shared__ u32 sDoc;
	__shared__ u32 sWave[ SORT_WAVES];
	const u32 tid = threadIdx.x, wave = tid >> 6;
	for (;;)
	{
		// the document comes to every wave of the workgroup through LDS: all of them take the same trips to the barriers below
		__syncthreads();
		if (tid == 0) sDoc = atomicAdd( P.sortCursor, 1u);
		__syncthreads();
		const u32 doc = sDoc;
		if (doc >= P.ndocs) break;
		const u64 rp = P.docResultOffsets[ doc];
		u64 nk = P.docResultOffsets[ doc+1] - rp;
		if (nk == 0 || rp + nk > P.nofResults) continue;
		SortDoc D = { P, 0, P.docRange[ 2*(u64)doc], (u32)P.docRange[ 2*(u64)doc+1]};
		if (D.n > P.nofResults || D.first > P.nofResults - D.n) continue;
		if (nk > D.n) nk = D.n;
		D.R = P.results + 9*D.first;
		u64* const key0 = P.sortKeys[ 0] + rp; u64* const key1 = P.sortKeys[ 1] + rp;
		u32* const idx0 = P.sortIdx[ 0] + rp; u32* const idx1 = P.sortIdx[ 1] + rp;

		if (P.exclusive)
		{
			// the survivors in the engine's order, with their ranks: staged in buffer 1 (the tiles below go to buffer 0)
			const uint8_t* C = P.covered + D.first;
			u32 rank0 = 0;
			for (u32 base=0; base<D.n; base+=SORT_THREADS)
			{
				const u32 ri = base + tid;
				const bool keep = ri < D.n && C[ ri] == 0;
				const u64 mask = __ballot( keep);
				if (LANE == 0) sWave[ wave] = (u32)__popcll( mask);
				__syncthreads();
				u32 before = 0, total = 0;
				for (u32 w=0; w<SORT_WAVES; ++w) { const u32 v = sWave[ w]; if (w < wave) before += v; total += v; }
				const u64 rank = (u64)rank0 + before + (u32)__popcll( mask & ((1ull << LANE) - 1ull));
				if (keep && rank < nk)
				{
					const u32* r = D.R + 9*(u64)ri;
					key1[ rank] = ((u64)r[ 1] << 32) | r[ 2]; idx1[ rank] = ri;
				}
				rank0 += total;
				__syncthreads();
			}
		}
		// tiles: a bitonic network over the next power of two, padded.  Distances of 64 and more are compare-exchanges in
		// LDS, a thread per pair on consecutive addresses (no two lanes of a half wave on one bank); the distances below
		// 64, where a pair per thread would step through LDS at a power-of-two stride, run in registers (waveStages).
		const u64 ntiles = (nk + FINISH_SORT_TILE - 1) / FINISH_SORT_TILE;
		for (u64 t=0; t<ntiles; ++t)
		{
			const u64 tb = t * FINISH_SORT_TILE;
			const u32 cnt = (u32)(nk - tb < FINISH_SORT_TILE ? nk - tb : FINISH_SORT_TILE);
			u32 m = 64;
			while (m < cnt) m <<= 1;
			for (u32 c=wave*64; c<m; c+=SORT_THREADS)
			{
				const u32 i = c + LANE;
				u64 key = ~0ull; u32 idx = NO_ENTRY;
				if (i < cnt)
				{
					if (P.exclusive) { key = key1[ tb + i]; idx = idx1[ tb + i]; }
					else { const u32* r = D.R + 9*(tb + i); key = ((u64)r[ 1] << 32) | r[ 2]; idx = (u32)(tb + i); }
				}
				for (u32 k=2; k<=64; k<<=1) waveStages( D, key, idx, i, k, k >> 1);
				K[ i] = key; I[ i] = idx;
			}
			__syncthreads();
			for (u32 k=128; k<=m; k<<=1)
			{
				for (u32 j=k>>1; j>=64; j>>=1)
				{
					for (u32 p=tid; p<(m>>1); p+=SORT_THREADS)
					{
						const u32 i = 2*j*(p / j) + (p % j);
						const u64 ka = K[ i], kb = K[ i+j];
						const u32 ia = I[ i], ib = I[ i+j];
						const bool asc = (i & k) == 0;
						if (asc ? entryLess( D, kb, ib, ka, ia) : entryLess( D, ka, ia, kb, ib))
						{
							K[ i] = kb; K[ i+j] = ka; I[ i] = ib; I[ i+j] = ia;
						}
					}
					__syncthreads();
				}
				for (u32 c=wave*64; c<m; c+=SORT_THREADS)
				{
					const u32 i = c + LANE;
					u64 key = K[ i]; u32 idx = I[ i];
					waveStages( D, key, idx, i, k, 32);
					K[ i] = key; I[ i] = idx;
				}
				__syncthreads();
			}
			for (u32 i=tid; i<cnt; i+=SORT_THREADS)
			{
				idx0[ tb + i] = I[ i];
				if (ntiles > 1) key0[ tb + i] = K[ i];		// (one tile: nothing is left to merge)
			}
			__syncthreads();
		}
		// merge passes between the two buffers: every thread takes MERGE_RUN outputs of a pair of runs, finds where they
		// begin in the two runs (merge path: a binary search on its diagonal) and merges them one by one
		u32 src = 0;
		for (u64 W=FINISH_SORT_TILE; W<nk; W<<=1, src^=1)
		{
			const u64* sk = src ? key1 : key0; const u32* si = src ? idx1 : idx0;
			u64* dk = src ? key0 : key1; u32* di = src ? idx0 : idx1;
			for (u64 o0=(u64)tid*MERGE_RUN; o0<nk; o0+=(u64)SORT_THREADS*MERGE_RUN)
			{
				const u64 pairStart = o0 / (2*W) * (2*W);
				const u64 aLen = nk - pairStart < W ? nk - pairStart : W;
				const u64 bBeg = pairStart + aLen;
				const u64 bLen = nk - bBeg < W ? nk - bBeg : W;
				const u64 diag = o0 - pairStart;
				const u64* ak = sk + pairStart; const u32* ai = si + pairStart;
				const u64* bk = sk + bBeg; const u32* bi = si + bBeg;
				u64 lo = diag > bLen ? diag - bLen : 0, hi = diag < aLen ? diag : aLen;
				while (lo < hi)
				{
					const u64 mid = (lo + hi) >> 1;
					if (entryLess( D, bk[ diag-1-mid], bi[ diag-1-mid], ak[ mid], ai[ mid])) hi = mid; else lo = mid + 1;
				}
				u64 a = lo, b = diag - lo;
				const u32 cnt = (u32)(nk - o0 < MERGE_RUN ? nk - o0 : MERGE_RUN);
				u64 ka = 0, kb = 0; u32 ia = 0, ib = 0;
				if (a < aLen) { ka = ak[ a]; ia = ai[ a]; }
				if (b < bLen) { kb = bk[ b]; ib = bi[ b]; }
				for (u32 o=0; o<cnt; ++o)
				{
					const bool takeA = b >= bLen || (a < aLen && !entryLess( D, kb, ib, ka, ia));
					if (takeA)
					{
						dk[ o0+o] = ka; di[ o0+o] = ia;
						if (++a < aLen) { ka = ak[ a]; ia = ai[ a]; }
					}
					else
					{
						dk[ o0+o] = kb; di[ o0+o] = ib;
						if (++b < bLen) { kb = bk[ b]; ib = bi[ b]; }
					}
				}
			}
			__syncthreads();
		}
	}
}

// ---- pass C in canonical order: a lane per result in sorted order, as the `exclusive` branch of placeDocuments
__device__ void placeSorted( const FinishParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 rp = uni64( P.docResultOffsets[ doc]), nk = uni64( P.docResultOffsets[ doc+1]) - rp;
		const u64 ip = uni64( P.docItemOffsets[ doc]), nki = uni64( P.docItemOffsets[ doc+1]) - ip;
		if (nk == 0) continue;
		if (rp + nk > P.nofResults || ip + nki > P.nofItems) continue;
		const u64 first = uni64( P.docRange[ 2*(u64)doc]);
		const u32 n = uni( (u32)P.docRange[ 2*(u64)doc+1]);
		if (n > P.nofResults || first > P.nofResults - n) continue;
		const u32* R = P.results + 9*first;
		const u32* perm = P.sortIdx[ sortLevels( nk) & 1] + rp;
		u64 iat = ip;
		for (u64 base=0; base<nk; base+=64)
		{
			const u64 e = base + LANE;
			const u32 ri = e < nk ? perm[ e] : NO_ENTRY;
			const bool ok = ri < n;
			const u32* r = R + 9*(u64)(ok ? ri : 0u);
			const u32 ib = ok ? r[ 7] : 0u, ic = ok ? r[ 8] : 0u;
			const u32 iincl = waveScanAdd( ic);
			const u64 myItems = iat + (iincl - ic);
			if (ok && myItems + ic <= ip + nki && (u64)ib + ic <= P.nofItems) placeResult( P, r, first + ri, rp + e, ib, ic, myItems);
			iat += uni( (u32)__shfl( (int)iincl, 63));
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_finish_count_kernel( FinishParams P) { countDocuments( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_finish_mark_kernel( FinishParams P) { markDocuments( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_finish_offsets_kernel( FinishParams P) { scanDocuments( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_finish_place_kernel( FinishParams P) { placeDocuments( P); }
extern "C" __global__ __launch_bounds__(SORT_THREADS) void spa_l2_finish_sort_kernel( FinishParams P) { sortDocuments( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_finish_place_sorted_kernel( FinishParams P) { placeSorted( P); }

namespace spa {
hipError_t launchL2Finish( const FinishParams& P, unsigned numCUs, hipStream_t stream, hipEvent_t* ev)
{
	const dim3 perDocument( wavePerDocumentBlocks( P.ndocs, numCUs));	// the passes that walk results
	hipError_t e;
	if (ev && (e = hipEventRecord( ev[ 0], stream)) != hipSuccess) return e;
	if (P.exclusive) hipLaunchKernelGGL( spa_l2_finish_mark_kernel, perDocument, dim3( 256), 0, stream, P);
	else
	{
		unsigned blocks = P.ndocs / 256 + 1;		// a thread per document, grid-stride beyond 1024 workgroups
		if (blocks > 1024) blocks = 1024;
		hipLaunchKernelGGL( spa_l2_finish_count_kernel, dim3( blocks), dim3( 256), 0, stream, P);
	}
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 1], stream)) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_finish_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 2], stream)) != hipSuccess) return e;
	if (P.canonical)
	{
		// a workgroup per document; the 48 KiB tile lets three of them share a CU's LDS
		const size_t groups = (size_t)numCUs * 3;
		hipLaunchKernelGGL( spa_l2_finish_sort_kernel, dim3( (unsigned)(P.ndocs < groups ? (P.ndocs ? P.ndocs : 1) : groups)), dim3( SORT_THREADS), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
		if (ev && (e = hipEventRecord( ev[ 4], stream)) != hipSuccess) return e;
		hipLaunchKernelGGL( spa_l2_finish_place_sorted_kernel, perDocument, dim3( 256), 0, stream, P);
	}
	else hipLaunchKernelGGL( spa_l2_finish_place_kernel, perDocument, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	if (ev && (e = hipEventRecord( ev[ 3], stream)) != hipSuccess) return e;
	return hipSuccess;
}
}
