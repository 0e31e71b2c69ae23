// Term passes of a finished device batch (l2_terms.h): count, offsets, place.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_terms.h"
#include "l2_term_value.h"

using namespace spa;

namespace {

enum {TERM_ERR_RANGE=5};		// SP_DOC_ERR_RANGE (include/strus_pattern_amd.h)
const u32 NONE = TERM_NONE;		// an empty slot, no slot, no term (l2_term_value.h: the value of a result, hashTerm, sameBytes, loadShared)

// What one lane wrote is read by the other lanes of its wave only across this (l2_freq_kernel.hip): the release is of
// agent scope, so that the stores have arrived where the atomics are executed.  Once per sweep, never per result.
__device__ __forceinline__ void waveSync()
{
	__builtin_amdgcn_fence( __ATOMIC_RELEASE, "agent");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "workgroup");
}

// ---- pass A: a wave per document
__device__ void countTerms( const TermsParams& P, u32* ldsTable)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( P.docOffsets[ doc]), r1 = uni64( P.docOffsets[ (u64)doc+1]);
		u32 count = 0;
		bool failed = false;
		if (r0 < r1 && r1 <= P.nresults && r1 - r0 >= 0x7FFFFFFFull) failed = true;	// (indices and slots are 32 bits)
		else if (r0 < r1 && r1 <= P.nresults)
		{
			const u32 n = (u32)(r1 - r0), m = 2*n;
			// a selected source that failed the document
			for (int s=0; s<2; ++s)
			{
				if ((P.flags & (1u << s)) && uni( (u32)P.source[ s].docStatus[ doc]) != 0) failed = true;
			}
			// the bound check of every handle, before anything is done with one
			for (u64 r=r0; !failed && r<r1; r+=64)
			{
				const u64 i = r + LANE;
				const bool active = i < r1;
				const u32 h = active ? P.results[ 9*i] : 0u;
				if (__ballot( active && !validHandle( P, h))) failed = true;
			}
			if (!failed)
			{
				u32* table = n <= (u32)TERM_TILE ? ldsTable : P.table + 2*r0;
				waveSync();		// (lanes may still be at the table of the document before)
				for (u32 k=LANE; k<m; k+=64) table[ k] = NONE;
				waveSync();
				// every result to the slot of its term; the slot is kept in `leader` until all are in
				bool bad = false;
				for (u64 r=r0; r<r1; r+=64)
				{
					const u64 at = r + LANE;
					if (at >= r1) continue;
					const u32 i = (u32)(at - r0);
					const u32 h = P.results[ 9*at];
					u32 found = NONE;
					const TermValue v = valueOf( P, at);
					if (!validHandle( P, h) || !v.ok) bad = true;
					else
					{
						u32 slot = (hashTerm( h, v) & P.hashMask) % m;
						for (u32 probes=0; probes<m; ++probes)
						{
							const u32 cur = atomicCAS( &table[ slot], NONE, i);
							if (cur == NONE) { found = slot; break; }
							if (cur < n && P.results[ 9*(r0 + cur)] == h)
							{
								const TermValue w = valueOf( P, r0 + cur);
								if (w.ok && w.len == v.len && sameBytes( v.p, w.p, v.len))
								{
									if (i < cur) atomicMin( &table[ slot], i);
									found = slot;
									break;
								}
							}
							slot = slot + 1 == m ? 0 : slot + 1;
						}
					}
					P.leader[ at] = found;
				}
				if (__ballot( bad)) failed = true;
				waveSync();
				// the smallest index of every term
				for (u64 r=r0; !failed && r<r1; r+=64)
				{
					const u64 at = r + LANE;
					const bool active = at < r1;
					const u32 i = (u32)(at - r0);
					u32 first = i;
					if (active)
					{
						const u32 slot = P.leader[ at];
						if (slot < m) first = atomicMin( &table[ slot], NONE);	// (a read where the atomics are executed)
						if (first > i) first = i;
						P.leader[ at] = first;
					}
					count += (u32)__popcll( __ballot( active && first == i));
				}
			}
		}
		if (LANE == 0)
		{
			P.docCount[ doc] = failed ? 0u : count;
			P.docStatus[ doc] = failed ? TERM_ERR_RANGE : 0;
		}
	}
}

// ---- pass B: the offsets of the documents' records (doc_passes.h).  A document with a range status counts 0.
__device__ void scanDocuments( const TermsParams& P)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.ndocs,
		[&]( u64 d) { return DocCounts<1>{{ P.docStatus[ d] == 0 ? P.docCount[ d] : 0u}}; },
		[&]( u64 d, const DocCounts<1>&, const DocSums<1>& at) { P.docTermOffsets[ d] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { P.docTermOffsets[ P.ndocs] = total; *P.total = total; }
}

// ---- pass C: a wave per document.  Whatever the results and the working arrays hold, every record written lies inside
// the document's block [docTermOffsets[d], docTermOffsets[d+1]) and that inside the output.
__device__ void placeTerms( const TermsParams& P, u32* histogram)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 1);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( P.docOffsets[ doc]), r1 = uni64( P.docOffsets[ (u64)doc+1]);
		if (r0 >= r1 || r1 > P.nresults) continue;
		const u32 n = r1 - r0 < 0x7FFFFFFFull ? (u32)(r1 - r0) : 0u;	// (0: pass A has failed the document)
		const u64 at = uni64( P.docTermOffsets[ doc]), end = uni64( P.docTermOffsets[ (u64)doc+1]);
		if (uni( (u32)P.docStatus[ doc]) != 0 || end <= at || end > P.capacity || end - at > n)
		{
			// a failed document: none of its results has a term
			for (u64 r=r0+LANE; r<r1; r+=64) P.resultTerm[ r] = NONE;
			continue;
		}
		const u32 nterms = (u32)(end - at);
		u32* records = P.records + 6*at;
		// the terms per handle
		waveSync();		// (the atomics on the histogram of the document before have returned; its stores are out)
		for (u32 k=LANE; k<P.handleBound; k+=64) histogram[ k] = 0;
		waveSync();
		for (u64 r=r0; r<r1; r+=64)
		{
			const u64 i = r + LANE;
			if (i >= r1 || P.leader[ i] != (u32)(i - r0)) continue;
			const u32 h = P.results[ 9*i];
			if (validHandle( P, h)) atomicAdd( &histogram[ h], 1u);
		}
		waveSync();
		// their exclusive prefix sums: the first record of every handle
		u32 carry = 0;
		for (u32 k0=0; k0<P.handleBound; k0+=64)
		{
			const u32 k = k0 + LANE;
			const u32 v = k < P.handleBound ? loadShared( &histogram[ k]) : 0u;
			const u32 incl = waveScanAdd( v);
			if (k < P.handleBound) histogram[ k] = carry + incl - v;
			carry += uni( (u32)__shfl( (int)incl, 63));
		}
		waveSync();
		// the leaders in index order: consecutive records behind the first of their handle
		for (u64 r=r0; r<r1; r+=64)
		{
			const u64 i = r + LANE;
			u32 h = 0;
			bool lead = i < r1 && P.leader[ i] == (u32)(i - r0);
			if (lead) { h = P.results[ 9*i]; lead = validHandle( P, h); }
			// the leaders of this trip with the same handle: the lowest lane speaks for them
			u32 speaker = LANE, rank = 0, members = 0;
			u64 todo = __ballot( lead);
			while (todo)
			{
				const int first = __ffsll( (unsigned long long)todo) - 1;
				const u32 h0 = uni( (u32)__shfl( (int)h, first));
				const bool mine = lead && h == h0;
				const u64 group = __ballot( mine);
				if (mine)
				{
					speaker = (u32)first;
					rank = (u32)__popcll( group & ((1ull << LANE) - 1ull));
					members = (u32)__popcll( group);
				}
				todo &= ~group;
			}
			u32 base = 0;
			if (lead && speaker == LANE) base = atomicAdd( &histogram[ h], members);
			base = (u32)__shfl( (int)base, (int)speaker);
			if (lead)
			{
				const u32 t = base + rank;
				const TermValue v = valueOf( P, i);
				if (t < nterms)
				{
					u32* rec = records + 6*(u64)t;
					rec[ 0] = h; rec[ 1] = 0; rec[ 2] = NONE; rec[ 3] = 0; rec[ 4] = (u32)(i - r0); rec[ 5] = v.len;
				}
				P.resultTerm[ i] = t < nterms ? t : NONE;
			}
		}
		waveSync();
		// every result to the term of its leader: its index, and count, minimum and maximum
		for (u64 r=r0; r<r1; r+=64)
		{
			const u64 i = r + LANE;
			if (i >= r1) continue;
			const u32 first = P.leader[ i];
			u32 t = NONE;
			if (first <= (u32)(i - r0)) t = loadShared( &P.resultTerm[ r0 + first]);
			if (t >= nterms) { P.resultTerm[ i] = NONE; continue; }
			if (first != (u32)(i - r0)) P.resultTerm[ i] = t;
			const u32x4 w = *(const u32x4u*)(P.results + 9*i);	// handle, ordpos, ordend
			u32* rec = records + 6*(u64)t;
			atomicAdd( rec + 1, 1u);
			atomicMin( rec + 2, w.y);
			atomicMax( rec + 3, w.z);
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_terms_count_kernel( TermsParams P)
{
	__shared__ u32 table[ 4][ 2*TERM_TILE];
	countTerms( P, table[ threadIdx.x >> 6]);
}

extern "C" __global__ __launch_bounds__(1024) void spa_l2_terms_offsets_kernel( TermsParams P) { scanDocuments( P); }

extern "C" __global__ __launch_bounds__(256) void spa_l2_terms_place_kernel( TermsParams P)
{
	const u64 wave = (u64)blockIdx.x*4 + (threadIdx.x >> 6);
	placeTerms( P, P.histogram + wave*P.handleBound);
}

namespace spa {

unsigned l2TermsWaves( size_t ndocs, unsigned numCUs) { return 4*wavePerDocumentBlocks( ndocs, numCUs); }

hipError_t launchL2TermsCount( const TermsParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	hipLaunchKernelGGL( spa_l2_terms_count_kernel, dim3( wavePerDocumentBlocks( P.ndocs, numCUs)), dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_terms_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	return hipGetLastError();
}

hipError_t launchL2TermsPlace( const TermsParams& P, unsigned numCUs, hipStream_t stream)
{
	hipLaunchKernelGGL( spa_l2_terms_place_kernel, dim3( wavePerDocumentBlocks( P.ndocs, numCUs)), dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
