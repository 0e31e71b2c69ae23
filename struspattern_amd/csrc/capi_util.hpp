// What the two halves of the C-ABI (capi_l1.cpp; capi_l2.cpp, capi_l2_finished.cpp) share: exception -> return code, text and blob export,
// the entry points that are the same for a lexer and a matcher context.
#ifndef SPA_CAPI_UTIL_HPP
#define SPA_CAPI_UTIL_HPP
#include "../../include/strus_pattern_amd.h"
#include "hip_util.hpp"
#include "batch_fetch.hpp"
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace spa {

// "at least one document failed": the batch is complete, its doc_status tells which ones (SP_ERR_MATCH)
struct DocumentFailed :public std::runtime_error
{
	explicit DocumentFailed( const std::string& msg) :std::runtime_error( msg){}
};

template <class FN>
int guardedCall( std::string& err, int errcode, FN fn)
{
	try { fn(); return SP_OK; }
	catch (const std::bad_alloc&) { err = "memory allocation error in strus pattern"; return SP_ERR_NOMEM; }
	catch (const HipError& e) { err = e.what(); return SP_ERR_DEVICE; }
	catch (const DocumentFailed& e) { err = e.what(); return SP_ERR_MATCH; }
	catch (const std::exception& e) { err = e.what(); return errcode; }
}

// bounded copy of a message into a caller's buffer (which may be absent)
inline void copyText( char* dst, size_t dstsize, const char* text)
{
	if (dst && dstsize) { std::strncpy( dst, text, dstsize-1); dst[ dstsize-1] = 0; }
}

// sp_*_serialize: what `save` writes as a blob for the caller (sp_free)
template <class FN>
int exportBlob( std::string& err, void** blob, size_t* size, FN save)
{
	*blob = 0; *size = 0;
	return guardedCall( err, SP_ERR_INVALID, [&]{
		std::vector<uint8_t> buf;
		save( buf);
		*blob = hostArray<uint8_t>( buf.size() ? buf.size() : 1);
		std::memcpy( *blob, buf.data(), buf.size());
		*size = buf.size();
	});
}

// sp_*_deserialize: a new handle that `load` has filled, or NULL with the message in `err`
template <class HANDLE, class FN>
HANDLE* importBlob( char* err, size_t errsize, FN load)
{
	HANDLE* h = 0;
	try { h = new HANDLE(); load( *h); return h; }
	catch (const std::exception& e) { copyText( err, errsize, e.what()); delete h; return 0; }
}

// what of a counted output lies inside its buffer
inline uint64_t clampCount( uint64_t counted, uint64_t capacity) { return counted < capacity ? counted : capacity; }

// the copies of a batch fetch (batch_fetch.hpp) from the device, on `stream`
inline auto deviceToHost( hipStream_t stream)
{
	return [stream]( void* dst, const void* src, size_t n){ copySync( stream, dst, src, n, hipMemcpyDeviceToHost); };
}

// ---- a pass sequence that runs behind the stage before it (the finish behind its batch, the text behind the finish, the
// stitch behind the lexer's batch): whether its output stands, the stream it ran on, and the N events between its passes
template <int N>
struct PassRun
{
	bool done = false;
	hipStream_t stream = 0;
	Event ev[ N]; bool evValid = false;

	// a run on `on`: another stream than the previous stage's runs behind the event that closes that stage
	void begin( hipStream_t on, hipStream_t prevStream, hipEvent_t prevEvent)
	{
		done = evValid = false;
		for (int i=0; i<N; ++i) ev[ i].create();
		if (on != prevStream) HIP_CHECK( hipStreamWaitEvent( on, prevEvent, 0));
	}
	// the events as the launch functions take them
	void events( hipEvent_t (&out)[ N]) const { for (int i=0; i<N; ++i) out[ i] = ev[ i]; }
	// every pass is launched and every event recorded
	void completed( hipStream_t on) { stream = on; done = evValid = true; }
	// milliseconds from event i to event j of the last run (waits for j): behind every sp_*_last_*_ms
	int ms( int i, int j, double* out) const
	{
		*out = -1.0;
		if (!evValid) return SP_ERR_INVALID;
		if (hipEventSynchronize( ev[ j]) != hipSuccess) return SP_ERR_DEVICE;
		return elapsedMs( ev[ i], ev[ j], *out) ? SP_OK : SP_ERR_DEVICE;
	}
};

// ---- sp_*_ctx_batch_status, sp_*_ctx_last_kernel_ms
template <class CTX>
int batchStatus( CTX* c, const DeviceBuffer& dDocStatus, int32_t* status, size_t ndocs)
{
	return guardedCall( c->lasterror, SP_ERR_DEVICE, [&]{
		HIP_CHECK( hipSetDevice( c->device));
		HIP_CHECK( hipStreamSynchronize( c->lastStream));
		if (ndocs > c->lastNdocs) ndocs = c->lastNdocs;
		if (ndocs) copySync( c->own, status, dDocStatus.ptr, ndocs*sizeof(int32_t), hipMemcpyDeviceToHost);
	});
}

template <class CTX>
double lastKernelMs( CTX* c)
{
	double ms = -1.0;
	if (!c->evValid || hipEventSynchronize( c->evStop) != hipSuccess || !elapsedMs( c->evStart, c->evStop, ms)) return -1.0;
	return ms;
}

} // namespace
#endif
