// Dictionary passes of a finished device batch (l2_dict.h): insert, resolve, offsets, place, accumulate.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_dict.h"
#include "l2_term_value.h"

using namespace spa;

namespace {

const u32 NONE = TERM_NONE;		// an empty slot, no slot, no leader, no entry

// the term records [t0, t1) of a document, wave-uniform; false: none that lie inside the N records
__device__ __forceinline__ bool documentRecords( const DictParams& P, u32 doc, u64& t0, u64& t1)
{
	t0 = uni64( P.docTermOffsets[ doc]); t1 = uni64( P.docTermOffsets[ (u64)doc+1]);
	return t0 < t1 && t1 <= P.nterms;
}

// The handle and the value of term record i (i < P.nterms) of document doc (doc < P.ndocs): the range of its first_result in
// the selected source.  false: a handle outside the bound, a first_result outside the document or the finished results, a
// range outside the source, or a value_bytes that is not the length of the range; nothing is read for it beyond the record.
__device__ __forceinline__ bool recordValue( const DictParams& P, u32 doc, u64 i, u32& handle, TermValue& v)
{
	const u64 r0 = P.docOffsets[ doc], r1 = P.docOffsets[ (u64)doc+1];
	const u32* rec = P.terms + 6*i;
	handle = rec[ 0];
	const u32 first = rec[ 4];
	v.p = 0; v.len = 0; v.ok = false;
	if (!(r0 <= r1 && r1 <= P.nresults && first < r1 - r0) || !validHandle( P, handle)) return false;
	v = valueOf( P, r0 + first);
	return v.ok && v.len == rec[ 5];
}

// the document of record i (i < P.nterms, P.ndocs >= 1): the last one whose records start at or before i, by the term
// offsets of an earlier launch; the caller checks that i lies inside it
__device__ __forceinline__ u32 documentOfRecord( const DictParams& P, u32 i)
{
	u32 lo = 0, hi = P.ndocs;
	while (hi - lo > 1)
	{
		const u32 mid = lo + (hi - lo)/2;
		if (P.docTermOffsets[ mid] <= i) lo = mid; else hi = mid;
	}
	return lo;
}

// ---- launch 1: every record to the slot of its term
__device__ void insertRecords( const DictParams& P)
{
	const u32 m = P.tableSlots;
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		u64 t0, t1;
		if (!documentRecords( P, doc, t0, t1)) continue;
		for (u64 t=t0; t<t1; t+=64)
		{
			const u64 at = t + LANE;
			if (at >= t1) continue;
			const u32 i = (u32)at;			// (N < 2^32 - 1)
			u32 h, found = NONE;
			TermValue v;
			if (recordValue( P, doc, at, h, v))
			{
				u32 slot = (hashTerm( h, v) & P.hashMask) % m;
				for (u32 probes=0; probes<m; ++probes)
				{
					const u32 cur = atomicCAS( &P.table[ slot], NONE, i);
					if (cur == NONE || cur == i) { found = slot; break; }
					if (cur < P.nterms && P.terms[ 6*(u64)cur] == h && P.terms[ 6*(u64)cur + 5] == v.len)
					{
						const u32 other = documentOfRecord( P, cur);
						u32 g;
						TermValue w;
						if (P.docTermOffsets[ other] <= cur && cur < P.docTermOffsets[ (u64)other+1]
						    && recordValue( P, other, cur, g, w) && sameBytes( v.p, w.p, v.len))
						{
							if (i < cur) atomicMin( &P.table[ slot], i);
							found = slot;
							break;
						}
					}
					slot = slot + 1 == m ? 0 : slot + 1;
				}
			}
			P.slot[ at] = found;
		}
	}
}

// ---- launch 2: the smallest record index of every term; the records that lead themselves, per document
__device__ void resolveLeaders( const DictParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 1);
		if (doc >= P.ndocs) break;
		u64 t0, t1;
		u32 count = 0;
		if (documentRecords( P, doc, t0, t1))
		{
			for (u64 t=t0; t<t1; t+=64)
			{
				const u64 at = t + LANE;
				const bool active = at < t1;
				u32 first = NONE;
				if (active)
				{
					const u32 slot = P.slot[ at];
					if (slot < P.tableSlots) first = loadShared( &P.table[ slot]);
					if (first > (u32)at) first = NONE;		// (a leader is the record itself or an earlier one)
					P.leader[ at] = first;
				}
				count += (u32)__popcll( __ballot( active && first == (u32)at));
			}
		}
		if (LANE == 0) P.docCount[ doc] = count;
	}
}

// ---- launch 3: the offsets of the documents' entries (doc_passes.h)
__device__ void scanDocuments( const DictParams& P)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.ndocs,
		[&]( u64 d) { return DocCounts<1>{{ P.docCount[ d]}}; },
		[&]( u64 d, const DocCounts<1>&, const DocSums<1>& at) { P.docDictOffsets[ d] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { P.docDictOffsets[ P.ndocs] = total; *P.total = total; }
}

// ---- launch 4: the leaders in record order behind the base of their document.  Every entry written lies inside
// [docDictOffsets[d], docDictOffsets[d+1]) and that inside the capacity.
__device__ void placeLeaders( const DictParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 2);
		if (doc >= P.ndocs) break;
		u64 t0, t1;
		if (!documentRecords( P, doc, t0, t1)) continue;
		const u64 base = uni64( P.docDictOffsets[ doc]), end = uni64( P.docDictOffsets[ (u64)doc+1]);
		const bool room = base <= end && end <= P.capacity && end <= MAX32;
		u64 next = base;
		for (u64 t=t0; t<t1; t+=64)
		{
			const u64 at = t + LANE;
			u32 h = 0;
			bool lead = at < t1 && P.leader[ at] == (u32)at;
			if (lead) { h = P.terms[ 6*at]; lead = validHandle( P, h); }
			const u64 leaders = __ballot( lead);
			const u64 e = next + (u32)__popcll( leaders & ((1ull << LANE) - 1ull));
			const bool placed = lead && room && e < end;
			if (placed)
			{
				u32* rec = P.records + 8*e;
				const u32x4 head = { h, P.terms[ 6*at + 5], doc, (u32)(at - t0)};
				const u32x4 zero = { 0u, 0u, 0u, 0u};
				*(u32x4*)rec = head;			// (an entry is 32 bytes and the records are 256-byte aligned)
				*(u32x4*)(rec + 4) = zero;
			}
			if (lead) P.termDict[ at] = placed ? (u32)e : NONE;
			next += (u32)__popcll( leaders);
			// the placed leaders of this trip with the same handle: the lowest lane adds their number
			u64 todo = __ballot( placed);
			while (todo)
			{
				const int first = __ffsll( (unsigned long long)todo) - 1;
				const u32 h0 = uni( (u32)__shfl( (int)h, first));
				const u64 group = __ballot( placed && h == h0);
				if (LANE == (u32)first) atomicAdd( &P.handleTerms[ h0], (u32)__popcll( group));
				todo &= ~group;
			}
		}
	}
}

// ---- launch 5: every record to the entry of its leader
__device__ void accumulateRecords( const DictParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor + 3);
		if (doc >= P.ndocs) break;
		u64 t0, t1;
		if (!documentRecords( P, doc, t0, t1)) continue;
		for (u64 t=t0+LANE; t<t1; t+=64)
		{
			const u32 first = P.leader[ t];
			u32 e = NONE;
			if (first <= (u32)t) e = P.termDict[ first];		// (written by launch 4, the record's own included)
			if (e >= P.capacity) { P.termDict[ t] = NONE; continue; }
			if (first != (u32)t) P.termDict[ t] = e;
			const u32 count = P.terms[ 6*t + 1];
			u32* rec = P.records + 8*(u64)e;
			atomicAdd( rec + 4, 1u);
			atomicMax( rec + 5, count);
			atomicAdd( (unsigned long long*)(rec + 6), (unsigned long long)count);
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_dict_insert_kernel( DictParams P) { insertRecords( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_dict_resolve_kernel( DictParams P) { resolveLeaders( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_dict_offsets_kernel( DictParams P) { scanDocuments( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_dict_place_kernel( DictParams P) { placeLeaders( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_dict_accumulate_kernel( DictParams P) { accumulateRecords( P); }

namespace spa {

hipError_t launchL2DictCount( const DictParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	const dim3 grid( wavePerDocumentBlocks( P.ndocs, numCUs));
	hipLaunchKernelGGL( spa_l2_dict_insert_kernel, grid, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_dict_resolve_kernel, grid, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_dict_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	return hipGetLastError();
}

hipError_t launchL2DictPlace( const DictParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	const dim3 grid( wavePerDocumentBlocks( P.ndocs, numCUs));
	hipLaunchKernelGGL( spa_l2_dict_place_kernel, grid, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL( spa_l2_dict_accumulate_kernel, grid, dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
