// The rule compiler handle and the GPU match context behind the C-ABI of level 2, shared by its two translation units:
// capi_l2.cpp (handle, context, batch launch, host entry points) and capi_l2_finished.cpp (what is made of a finished batch).
// capi_segment.cpp reads the two block products of a context through it (sp_segment_from_ctx).
#ifndef SPA_CAPI_L2_CTX_HPP
#define SPA_CAPI_L2_CTX_HPP
#include "l2_plan.hpp"
#include "result_values.hpp"
#include "capi_util.hpp"
#include <mutex>

using namespace spa;	// (the two handles are global names of the C header; this header is only for the files above)

struct sp_matcher
{
	RuleCompiler compiler;
	bool compiled = false;	// compile() is optional for the matcher (reference: tests/randomTokenPatternMatch :317-320)
	mutable std::string lasterror;
	// the parts of the format strings (result_values.hpp): built when the rule set compiles or is loaded, else at the first values call
	mutable std::mutex formatMutex;
	mutable FormatTable formatTable;
	mutable bool haveFormatTable = false;
	mutable size_t formatTableVariables = 0;	// the variable names the table was resolved against

	// rebuild = true (every compile, every load): the definitions may have changed under the same counts
	const FormatTable& formats( bool rebuild = false) const
	{
		std::lock_guard<std::mutex> lock( formatMutex);
		const size_t nvariables = compiler.variables().names().size();
		if (rebuild || !haveFormatTable || formatTable.count != compiler.formatCount() || formatTableVariables != nvariables)
		{
			formatTableVariables = nvariables;
			formatTable = buildFormatTable( compiler.formatCount(),
				[this]( uint32_t f) { return compiler.formatString( f); },
				[this]( const std::string& name) { return compiler.variables().get( name); });
			haveFormatTable = true;
		}
		return formatTable;
	}
};

struct sp_matcher_ctx
{
	const sp_matcher* inst = 0;
	int device = 0;
	unsigned numCUs = 256;
	L2Switches sw;		// read when the context is created
	L2EngineKind kind = L2_GENERAL;
	std::string lasterror;
	// the exact engine (l2_kernel.hip): compiled tables, working memory, the documents of a launch in list mode
	struct Exact
	{
		DeviceBuffer dPrograms, dTrigdefs, dKeytab, dKeylist, dDocList;
		uint32_t keymask = 0, nofStopWords = 0;
		ArenaLayout layout = initialArena();
		CountedBuffer arena;		// count: waves; 0 forces a new layout at the next launch
	} exact;
	// flat tier (l2_fast.h): flat rule sets run with their hot state in LDS; the general kernel takes what it hands over
	struct Flat
	{
		bool on = false;
		std::string whyNot;
		DeviceBuffer dKeyinst, dStatics;
		FlatPlan plan;		// kernel instance = LDS capacities (l2_fast_kernel.hip), spill layout
		CountedBuffer spill;		// count: waves
		unsigned blocksPerCU = 0;
	} flat;
	// result-set mode (l2_join.h; SP_CTX_RESULT_SETS or SPA_L2_JOIN=1): result multisets without materialised rule instances
	struct ResultSets
	{
		bool on = false, altRules = false;
		std::string whyNot;
		uint32_t keymask = 0, maxRange = 0, delimiter = 0;
		DeviceBuffer dKeytab, dRules, dFilter, dCounts;
	} join;
	// batch buffers (grown on demand): the input of the host entry points, the output of every rule kernel
	struct BatchIO
	{
		DeviceBuffer dCursor, dCounters;
		DeviceBuffer dLexems, dOrigseg, dDocOffsets;
		CountedBuffer results, items;	// count: sp_result_t, sp_result_item_t
		DeviceBuffer dDocRange, dDocStats, dDocStatus;
		DeviceBuffer dResultFormat, dItemFormat;	// only for matchers with format strings
		bool withFormats = false, withItems = true;
		uint64_t minResults = 0, minItems = 0;
	} io;
	// the last batch finished on the device (l2_finish.h); nothing is allocated before the first sp_matcher_ctx_batch_finish_device
	struct Finished
	{
		PassRun<5> run;		// ev[4]: between the sort and the placement of a canonical finish
		DeviceBuffer dResults, dItems, dResultFormat, dItemFormat, dDocResultOffsets, dDocItemOffsets, dTotals, dKept, dCovered, dCursor;
		bool canonical = false;
		// working memory of the canonical order, allocated at the first finish that asks for it
		DeviceBuffer dSortKeys[ 2], dSortIdx[ 2], dSortCursor;
	};
	// what the matched text (l2_text.h) and the values of the format strings (l2_values.h) keep alike: bytes per record of a
	// family, [0] results, [1] items; nothing is allocated before the first call
	struct ByteFamilies
	{
		PassRun<2> run;
		DeviceBuffer dBytes[ 2], dOffsets[ 2], dWork[ 2], dDocBytes[ 2], dDocOffsets[ 2];
		DeviceBuffer dStatus, dTotals, dCursor;
		uint32_t flags = 0;
		size_t ndocs = 0;
		uint64_t nrecords[ 2] = {0, 0}, totals[ 2] = {0, 0};
	};
	struct Values :public ByteFamilies
	{
		DeviceBuffer dFmtParts, dParts, dPool;		// the format table, uploaded at the first call
		bool uploaded = false;
		uint32_t poolBytes = 0;
	};
	// the pattern frequencies of the last finished batch (l2_freq.h); nothing is allocated before the first sp_matcher_ctx_finished_pattern_freq_device
	struct Freq
	{
		PassRun<2> run;
		DeviceBuffer dRecords, dDocOffsets, dStatus, dHandleResults, dHandleDocs, dTotals, dDocCount, dDocMeta, dCursor;
		size_t ndocs = 0;
		uint32_t handleBound = 0;
		uint64_t total = 0;
	};
	// the index terms of the last finished batch (l2_terms.h); nothing is allocated before the first sp_matcher_ctx_finished_terms_device
	struct Terms
	{
		PassRun<2> run;
		DeviceBuffer dRecords, dDocOffsets, dResultTerm, dStatus, dTotals, dLeader, dTable, dHistogram, dDocCount, dCursor;
		size_t ndocs = 0;
		uint32_t handleBound = 0, flags = 0;
		uint64_t nresults = 0, total = 0;
	};
	// the dictionary of the last terms batch (l2_dict.h); nothing is allocated before the first sp_matcher_ctx_finished_dictionary_device
	struct Dict
	{
		PassRun<2> run;
		DeviceBuffer dRecords, dTermDict, dDocOffsets, dHandleTerms, dTotals, dTable, dSlot, dLeader, dDocCount, dCursor;
		size_t ndocs = 0;
		uint32_t handleBound = 0, flags = 0;
		uint64_t nterms = 0, total = 0;
	};
	// the postings of the last dictionary (l2_postings.h); nothing is allocated before the first sp_matcher_ctx_finished_postings_device
	struct Postings
	{
		PassRun<2> run;
		DeviceBuffer dPostings, dEntryOffsets, dRecordPosting, dTotals, dDocOf, dPairs[ 2], dHist, dCursor;
		size_t ndocs = 0;
		uint64_t nterms = 0, ndict = 0;
	};
	// the positions of the last postings (l2_positions.h); nothing is allocated before the first sp_matcher_ctx_finished_positions_device
	struct Positions
	{
		PassRun<2> run;
		DeviceBuffer dOccurrences, dPostingOffsets, dPostingPositions, dTotals, dDocOf, dPairs[ 2], dHist, dCursor;
		size_t ndocs = 0;
		uint64_t nterms = 0, nocc = 0;
		// diagnostics (sp_test_positions_launch_events): an event behind every launch of the last call, and its kind
		std::vector<Event> launchEv;
		std::vector<hipEvent_t> launchEvHandles;
		std::vector<int> launchKind;
		size_t launches = 0;
	};
	// the order of the last dictionary (l2_dictorder.h); nothing is allocated before the first sp_matcher_ctx_finished_dictionary_order_device
	struct DictOrder
	{
		PassRun<2> run;
		DeviceBuffer dOrder, dRank, dPrefixBytes, dHandleOffsets, dTotals, dKeys[ 2], dIndex[ 2], dValueAt, dValueLen, dCursor;
		uint32_t handleBound = 0;
		uint64_t ndict = 0;
	};
	// the term blocks of the last order (l2_termblocks.h); nothing is allocated before the first sp_matcher_ctx_finished_term_blocks_device
	struct TermBlocks
	{
		PassRun<2> run;
		DeviceBuffer dBytes, dBlockOffsets, dBlockHandles, dTotals, dBlockSize, dCursor;
		uint32_t blockEntries = 0;
		uint64_t ndict = 0, nblocks = 0, nbytes = 0;
	};
	// the posting blocks of the last order, postings and positions (l2_postingblocks.h); nothing is allocated before the first
	// sp_matcher_ctx_finished_posting_blocks_device
	struct PostingBlocks
	{
		PassRun<2> run;
		DeviceBuffer dBytes, dBlockOffsets, dTotals, dListOffsets, dListStart, dPostingBytes, dBlockSize, dCursor;
		uint32_t blockEntries = 0;
		uint64_t ndict = 0, nblocks = 0, nbytes = 0;
	};
	// the finish of the last batch and everything made of it (capi_l2_finished.cpp).  A product is a member here and is listed in drop().
	struct Products
	{
		Finished fin;
		ByteFamilies txt;
		Values val;
		Freq frq;
		Terms trm;
		Dict dct;
		Postings pst;
		Positions pos;
		DictOrder ord;
		TermBlocks blk;
		PostingBlocks pbk;
		// a new batch, a new finish: what stands here is of the one before
		void drop() { fin.run.done = false; txt.run.done = false; val.run.done = false; frq.run.done = false; trm.run.done = false; dropDictionary(); }
		// a new terms call: a dictionary is that of the terms it was built from, and postings are those of their dictionary
		void dropDictionary() { dct.run.done = false; dropPostings(); }
		// a new dictionary call: postings and an order are those of the dictionary they were built from, positions those of their
		// postings (postings and order do not touch each other)
		void dropPostings() { pst.run.done = false; dropPositions(); dropOrder(); }
		// a new postings call: positions are those of the postings they were built from, posting blocks those of their positions
		void dropPositions() { pos.run.done = false; pbk.run.done = false; }
		// a new order call: term blocks and posting blocks are those of the order they were built from
		void dropOrder() { ord.run.done = false; blk.run.done = false; pbk.run.done = false; }
	} prod;
	// single-document mode
	struct SingleDoc
	{
		std::vector<sp_lexem_t> lexems;
		std::vector<uint32_t> origseg; bool hasSeg = false;
		std::vector<uint32_t> resultFormat, itemFormat;	// of the last sp_matcher_ctx_fetch_results
		sp_matcher_stats_t stats = {};
	} cur;
	// the last launch
	bool haveBatch = false;
	size_t lastNdocs = 0;
	hipStream_t lastStream = 0;
	Event evStart, evStop; bool evValid = false;
	Stream own;		// the context's own stream (non-blocking): see sp_lexer_ctx; last member: it waits for its work before anything else goes
};

namespace spa {

// the counters of the last batch (its stream has been waited for), and what of its output lies inside the buffers
struct BatchCounts { uint64_t counters[ SPC_COUNT]; uint64_t results, items; };
inline BatchCounts readCounts( sp_matcher_ctx* c)
{
	BatchCounts b;
	copySync( c->own, b.counters, c->io.dCounters.ptr, sizeof(b.counters), hipMemcpyDeviceToHost);
	b.results = clampCount( b.counters[ SPC_RESULTS], c->io.results.count);
	b.items = clampCount( b.counters[ SPC_ITEMS], c->io.items.count);
	return b;
}

// grow-only, a failure is SP_ERR_NOMEM (the buffer is left empty, the context usable)
inline void reserveOrNoMem( DeviceBuffer& buf, size_t n)
{
	try { buf.reserve( n); }
	catch (const HipError&) { (void)hipGetLastError(); throw std::bad_alloc(); }
}

inline void requireFinished( const sp_matcher_ctx* c)
{
	if (!c->prod.fin.run.done) throw std::runtime_error( "the last batch of this context has not been finished (sp_matcher_ctx_batch_finish_device)");
}

// ---- One call that makes a product of the finished batch on `stream`: counting passes, one wait of the host for what they
// counted, placing passes that nobody waits for.  The steps every product shares; its buffers, parameters and `out` are its own.
struct ProductCall
{
	sp_matcher_ctx* c;
	PassRun<2>& run;
	hipStream_t stream;
	size_t ndocs;
	uint64_t finished[ 2];		// results, items of the finished batch

	// drops the product's last run and waits for the finish, whose totals size the working arrays
	ProductCall( sp_matcher_ctx* c_, PassRun<2>& run_, void* stream_)
		:ProductCall( c_, run_, stream_, Sized())
	{
		HIP_CHECK( hipStreamSynchronize( c->prod.fin.run.stream));
		copySync( c->own, finished, c->prod.fin.dTotals.ptr, sizeof(finished), hipMemcpyDeviceToHost);
	}
	// the same for a product whose sizes the host read at an earlier call: nothing is waited for, `finished` stays zero
	struct Sized {};
	ProductCall( sp_matcher_ctx* c_, PassRun<2>& run_, void* stream_, Sized)
		:c(c_),run(run_),stream((hipStream_t)stream_),ndocs(c_->lastNdocs),finished{ 0, 0}
	{
		requireFinished( c);
		HIP_CHECK( hipSetDevice( c->device));
		run.done = run.evValid = false;
	}
	// after the product's other reserves, before anything goes to the stream: another stream than the finish's runs behind the
	// finish; the status per document, the totals (u64) and the cursor (u32) that every product has start at zero
	void begin( DeviceBuffer& dStatus, DeviceBuffer& dTotals, size_t ntotals, DeviceBuffer& dCursor, size_t ncursor)
	{
		reserveOrNoMem( dStatus, (ndocs+1)*sizeof(int32_t));
		beginBehind( c->prod.fin.run.stream, c->prod.fin.run.ev[ 3], dTotals, ntotals, dCursor, ncursor);
		HIP_CHECK( hipMemsetAsync( dStatus.ptr, 0, (ndocs+1)*sizeof(int32_t), stream));
	}
	// the same without a status, behind the stage that ran on `prevStream` and closed with `prevEvent`
	void beginBehind( hipStream_t prevStream, hipEvent_t prevEvent, DeviceBuffer& dTotals, size_t ntotals, DeviceBuffer& dCursor, size_t ncursor)
	{
		reserveOrNoMem( dTotals, ntotals*sizeof(uint64_t));
		reserveOrNoMem( dCursor, ncursor*sizeof(uint32_t));
		run.begin( stream, prevStream, prevEvent);
		HIP_CHECK( hipMemsetAsync( dCursor.ptr, 0, ncursor*sizeof(uint32_t), stream));
		HIP_CHECK( hipMemsetAsync( dTotals.ptr, 0, ntotals*sizeof(uint64_t), stream));
	}
	// count, read the n totals counted, let `sized` reserve the output for them (it fills P in), place
	template <class PARAMS, class SIZED>
	void passes( PARAMS& P, hipError_t (*count)( const PARAMS&, unsigned, hipStream_t), hipError_t (*place)( const PARAMS&, unsigned, hipStream_t),
		     const DeviceBuffer& dTotals, uint64_t* totals, size_t n, SIZED sized)
	{
		HIP_CHECK( hipEventRecord( run.ev[ 0], stream));
		HIP_CHECK( count( P, c->numCUs, stream));
		HIP_CHECK( hipStreamSynchronize( stream));
		copySync( c->own, totals, dTotals.ptr, n*sizeof(uint64_t), hipMemcpyDeviceToHost);
		sized();
		HIP_CHECK( place( P, c->numCUs, stream));
		HIP_CHECK( hipEventRecord( run.ev[ 1], stream));
		run.completed( stream);
	}
};

} // namespace
#endif
