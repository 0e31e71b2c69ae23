// Position passes of a finished device batch (l2_positions.h): keys, offsets, rekey, place; the radix passes between them are
// those of radix_passes.h.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_positions.h"

using namespace spa;

namespace {

const u32 NONE = 0xFFFFFFFFu;

__device__ __forceinline__ u32 keyOf( u64 pair) { return (u32)pair; }
__device__ __forceinline__ u32 resultOf( u64 pair) { return (u32)(pair >> 32); }

// the term records of a document: their first index and their number, 0 where the offsets are not those of N records
__device__ __forceinline__ u32 documentRecords( const PositionsParams& P, u32 doc, u64& t0)
{
	t0 = P.docTermOffsets[ doc];
	const u64 t1 = P.docTermOffsets[ (u64)doc+1];
	return (t0 <= t1 && t1 <= P.nterms) ? (u32)(t1 - t0) : 0;	// (N < 2^32 - 1)
}

// ---- keys: the document and the pair of every result; the participants and their largest position
__device__ void writeKeys( const PositionsParams& P)
{
	u32 count = 0, largest = 0;
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		const u64 r0 = uni64( P.docOffsets[ doc]), r1 = uni64( P.docOffsets[ (u64)doc+1]);
		if (!(r0 < r1 && r1 <= P.nresults)) continue;
		u64 t0;
		const u32 nrecords = documentRecords( P, doc, t0);
		for (u64 r=r0+LANE; r<r1; r+=64)
		{
			const bool participates = P.resultTerm[ r] < nrecords;	// (0xFFFFFFFF is below no count)
			const u32 ordpos = P.results[ 9*r + 1];
			P.docOf[ r] = doc;
			P.pairs[ 0][ r] = ((u64)(u32)r << 32) | (participates ? ordpos : 0u);	// (nresults < 2^32 - 1)
			if (participates) { ++count; largest = ordpos > largest ? ordpos : largest; }
		}
	}
	// (a sum and a maximum: whatever the order of the waves)
	const u32 waveCount = waveScanAdd( count), waveLargest = waveScanMax( largest);
	if (LANE == 63 && waveCount)
	{
		atomicAdd( (unsigned long long*)&P.totals[ 0], (unsigned long long)waveCount);
		atomicMax( (unsigned long long*)&P.totals[ 2], (unsigned long long)waveLargest);
	}
}

// ---- offsets: where the list of every posting starts
__device__ void scanPostings( const PositionsParams& P)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.nterms,
		[&]( u64 p) { return DocCounts<1>{{ P.postings[ 4*p + 2]}}; },
		[&]( u64 p, const DocCounts<1>&, const DocSums<1>& at) { P.postingOffsets[ p] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) P.postingOffsets[ P.nterms] = total;
}

// ---- rekey: the key of every pair becomes the posting of its result, in place
__device__ void rekeyPairs( const PositionsParams& P)
{
	u64* buf = P.pairs[ P.passes[ 0] & 1];
	for (;;)
	{
		const u32 tile = nextDocument( P.cursor + 1);
		if (tile >= P.tiles) break;
		u64 q0, q1;
		radixTilePairs( P.nresults, tile, q0, q1);
		for (u64 q=q0+LANE; q<q1; q+=64)
		{
			const u32 r = resultOf( buf[ q]);
			u32 key = (u32)P.nterms;		// (the sentinel: behind every posting)
			if (r < P.nresults)
			{
				const u32 doc = P.docOf[ r];
				if (doc < P.ndocs)
				{
					u64 t0;
					const u32 nrecords = documentRecords( P, doc, t0);
					const u32 term = P.resultTerm[ r];
					if (term < nrecords)
					{
						const u32 p = P.recordPosting[ t0 + term];
						if (p < P.nterms) key = p;
					}
				}
			}
			buf[ q] = ((u64)r << 32) | key;
		}
	}
}

// ---- place: the occurrence of every sorted slot below nocc, and the distinct positions of every posting
__device__ void placeOccurrences( const PositionsParams& P)
{
	const u64* src = P.pairs[ (P.passes[ 0] + P.passes[ 1]) & 1];
	const u64 nocc = P.nocc < P.nresults ? P.nocc : P.nresults;
	for (;;)
	{
		const u32 tile = nextDocument( P.cursor + 2);
		if (tile >= P.tiles) break;
		u64 q0, q1;
		radixTilePairs( P.nresults, tile, q0, q1);
		if (q1 > nocc) q1 = nocc;
		u32 firsts = 0;
		for (u64 t=q0; t<q1; t+=64)
		{
			const u64 q = t + LANE;
			const bool active = q < q1;
			u32 posting = NONE, ordpos = NONE, result = NONE;
			if (active)
			{
				const u64 pair = src[ q];
				const u32 r = resultOf( pair);
				if (r < P.nresults && keyOf( pair) < P.nterms)
				{
					const u32 doc = P.docOf[ r];
					if (doc < P.ndocs && P.docOffsets[ doc] <= r)
					{
						posting = keyOf( pair); ordpos = P.results[ 9*(u64)r + 1]; result = r - (u32)P.docOffsets[ doc];
					}
				}
				*(u64*)(P.occurrences + 2*q) = ((u64)result << 32) | ordpos;	// (an occurrence is 8 bytes and the occurrences are 256-byte aligned)
			}
			const bool valid = posting != NONE;
			// the slot before: the lane below, for lane 0 the last slot of the trip before
			const u32 lanePosting = (u32)__shfl_up( (int)posting, 1);
			u32 prevPosting = lanePosting, prevOrdpos = (u32)__shfl_up( (int)ordpos, 1);
			if (LANE == 0)
			{
				prevPosting = NONE; prevOrdpos = NONE;
				if (active && q > 0)
				{
					const u64 pair = src[ q-1];
					if (resultOf( pair) < P.nresults && keyOf( pair) < P.nterms) { prevPosting = keyOf( pair); prevOrdpos = P.results[ 9*(u64)resultOf( pair) + 1]; }
				}
			}
			const bool first = valid && !(prevPosting == posting && prevOrdpos == ordpos);
			// the firsts of this trip with the same posting: the slots are sorted, so they are one run of lanes, and the lowest lane
			// of the run adds their number
			const u64 firstLanes = __ballot( first);
			const u64 runStarts = __ballot( LANE == 0 || lanePosting != posting);
			if (valid && (LANE == 0 || lanePosting != posting))
			{
				const u64 above = runStarts & ~((2ull << LANE) - 1ull);
				const u64 upTo = above ? ((1ull << (__ffsll( (unsigned long long)above) - 1)) - 1ull) : ~0ull;
				const u32 n = (u32)__popcll( firstLanes & upTo & ~((1ull << LANE) - 1ull));
				if (n) atomicAdd( &P.postingPositions[ posting], n);		// (a sum, whatever the order)
			}
			firsts += (u32)__popcll( firstLanes);
		}
		if (LANE == 0 && firsts) atomicAdd( (unsigned long long*)&P.totals[ 1], (unsigned long long)firsts);
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_positions_keys_kernel( PositionsParams P) { writeKeys( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_positions_offsets_kernel( PositionsParams P) { scanPostings( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_positions_rekey_kernel( PositionsParams P) { rekeyPairs( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_positions_place_kernel( PositionsParams P) { placeOccurrences( P); }

namespace spa {

namespace {
// diagnostics: an event behind the launch just enqueued (POS_NONE: in front of the first launch after the host's wait)
hipError_t mark( const PositionsParams& P, int kind, hipStream_t stream)
{
	PositionsLaunchEvents* t = P.events;
	if (!t || t->n >= t->capacity) return hipSuccess;
	t->kind[ t->n] = kind;
	return hipEventRecord( t->ev[ t->n++], stream);
}
}

hipError_t launchL2PositionsCount( const PositionsParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	if ((e = mark( P, POS_NONE, stream)) != hipSuccess) return e;
	if (P.nresults)
	{
		hipLaunchKernelGGL( spa_l2_positions_keys_kernel, dim3( wavePerDocumentBlocks( P.ndocs, numCUs)), dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess || (e = mark( P, POS_KEYS, stream)) != hipSuccess) return e;
	}
	hipLaunchKernelGGL( spa_l2_positions_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	return mark( P, POS_OFFSETS, stream);
}

hipError_t launchL2PositionsPlace( const PositionsParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	if (!P.nocc) return hipSuccess;		// (no occurrence: the offsets are all there is)
	if ((e = mark( P, POS_NONE, stream)) != hipSuccess) return e;
	const dim3 perTile( wavePerDocumentBlocks( P.tiles, numCUs));
	u32 pass = 0;
	for (int group=0; group<2; ++group)
	{
		for (u32 i=0; i<P.passes[ group]; ++i, ++pass)
		{
			RadixPass R;
			R.src = P.pairs[ pass & 1]; R.dst = P.pairs[ (pass & 1) ^ 1]; R.count = P.nresults; R.tiles = P.tiles;
			R.digitBits = P.digitBits; R.shift = i * P.digitBits; R.hist = P.hist; R.cursor = P.cursor + 3 + 2*pass;
			PositionsLaunchEvents* t = P.events;
			hipEvent_t* ev = (t && t->n + 3 <= t->capacity) ? t->ev + t->n : 0;
			if ((e = launchRadixPass( R, numCUs, stream, ev)) != hipSuccess) return e;
			if (ev) { t->kind[ t->n] = POS_HISTOGRAM; t->kind[ t->n+1] = POS_SCAN; t->kind[ t->n+2] = POS_SCATTER; t->n += 3; }
		}
		if (group == 0)
		{
			hipLaunchKernelGGL( spa_l2_positions_rekey_kernel, perTile, dim3( 256), 0, stream, P);
			if ((e = hipGetLastError()) != hipSuccess || (e = mark( P, POS_REKEY, stream)) != hipSuccess) return e;
		}
	}
	hipLaunchKernelGGL( spa_l2_positions_place_kernel, perTile, dim3( 256), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	return mark( P, POS_PLACE, stream);
}

}
