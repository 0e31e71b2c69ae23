// Postings passes of a finished device batch (l2_postings.h): keys, offsets, place; the radix passes between them (histogram /
// scan / scatter) are those of radix_passes.h.
#include <hip/hip_runtime.h>
#include "doc_passes.h"
#include "l2_postings.h"

using namespace spa;

namespace {

const u32 NONE = 0xFFFFFFFFu;

// a pair: the key in the low word, the record index in the high one
__device__ __forceinline__ u32 recordOf( u64 pair) { return (u32)(pair >> 32); }

// ---- keys: the document and the pair of every record
__device__ void writeKeys( const PostingsParams& P)
{
	for (;;)
	{
		const u32 doc = nextDocument( P.cursor);
		if (doc >= P.ndocs) break;
		const u64 t0 = uni64( P.docTermOffsets[ doc]), t1 = uni64( P.docTermOffsets[ (u64)doc+1]);
		if (!(t0 < t1 && t1 <= P.nterms)) continue;
		for (u64 t=t0+LANE; t<t1; t+=64)
		{
			u32 key = P.termDict[ t];
			if (key >= P.ndict) key = P.ndict - 1;		// (N >= 1 here and the host launches this for ndict >= 1 only)
			P.docOf[ t] = doc;
			P.pairs[ 0][ t] = ((u64)(u32)t << 32) | key;	// (N < 2^32 - 1)
		}
	}
}

// ---- offsets: where the list of every entry starts
__device__ void scanEntries( const PostingsParams& P)
{
	const u64 total = scanDocumentCounts<u64, 1>( P.ndict,
		[&]( u64 e) { return DocCounts<1>{{ P.dictRecords[ 8*e + 4]}}; },
		[&]( u64 e, const DocCounts<1>&, const DocSums<1>& at) { P.entryOffsets[ e] = at.v[ 0]; }).v[ 0];
	if (threadIdx.x == 0) { P.entryOffsets[ P.ndict] = total; *P.total = total; }
}

// ---- place: the posting of every sorted position, and the way back from its record
__device__ void placePostings( const PostingsParams& P)
{
	const u64* src = P.pairs[ P.passes & 1];
	for (;;)
	{
		const u32 tile = nextDocument( P.cursor + 1);
		if (tile >= P.tiles) break;
		u64 r0, r1;
		radixTilePairs( P.nterms, tile, r0, r1);
		for (u64 p=r0+LANE; p<r1; p+=64)
		{
			const u32 i = recordOf( src[ p]);
			u32x4 posting = { NONE, NONE, NONE, NONE};
			if (i < P.nterms)
			{
				const u32 doc = P.docOf[ i];
				if (doc < P.ndocs)
				{
					const u32* rec = P.terms + 6*(u64)i;
					posting.x = doc; posting.y = i - (u32)P.docTermOffsets[ doc]; posting.z = rec[ 1]; posting.w = rec[ 2];
					P.recordPosting[ i] = (u32)p;
				}
			}
			*(u32x4*)(P.postings + 4*p) = posting;		// (a posting is 16 bytes and the postings are 256-byte aligned)
		}
	}
}

} // anonymous namespace

extern "C" __global__ __launch_bounds__(256) void spa_l2_postings_keys_kernel( PostingsParams P) { writeKeys( P); }
extern "C" __global__ __launch_bounds__(1024) void spa_l2_postings_offsets_kernel( PostingsParams P) { scanEntries( P); }
extern "C" __global__ __launch_bounds__(256) void spa_l2_postings_place_kernel( PostingsParams P) { placePostings( P); }

namespace spa {

hipError_t launchL2Postings( const PostingsParams& P, unsigned numCUs, hipStream_t stream)
{
	hipError_t e;
	const bool records = P.nterms && P.ndict;	// (without records there are no entries: the offsets are the single 0 and the total)
	const dim3 perTile( wavePerDocumentBlocks( P.tiles, numCUs));
	if (records)
	{
		hipLaunchKernelGGL( spa_l2_postings_keys_kernel, dim3( wavePerDocumentBlocks( P.ndocs, numCUs)), dim3( 256), 0, stream, P);
		if ((e = hipGetLastError()) != hipSuccess) return e;
	}
	hipLaunchKernelGGL( spa_l2_postings_offsets_kernel, dim3( 1), dim3( 1024), 0, stream, P);
	if ((e = hipGetLastError()) != hipSuccess || !records) return e;
	for (u32 pass=0; pass<P.passes; ++pass)
	{
		RadixPass R;
		R.src = P.pairs[ pass & 1]; R.dst = P.pairs[ (pass & 1) ^ 1]; R.count = P.nterms; R.tiles = P.tiles;
		R.digitBits = P.digitBits; R.shift = pass * P.digitBits; R.hist = P.hist; R.cursor = P.cursor + 2 + 2*pass;
		if ((e = launchRadixPass( R, numCUs, stream)) != hipSuccess) return e;
	}
	hipLaunchKernelGGL( spa_l2_postings_place_kernel, perTile, dim3( 256), 0, stream, P);
	return hipGetLastError();
}

}
