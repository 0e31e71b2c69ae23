// Small HIP host helpers: error -> exception, RAII device buffer, owned stream and events.
#ifndef SPA_HIP_UTIL_HPP
#define SPA_HIP_UTIL_HPP
#include <hip/hip_runtime_api.h>
#include <stdexcept>
#include <string>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <atomic>

namespace spa {

struct HipError :public std::runtime_error
{
	explicit HipError( const std::string& msg) :std::runtime_error( msg){}
};

#define HIP_CHECK( EXPR) do { hipError_t e_ = (EXPR); if (e_ != hipSuccess) \
	throw spa::HipError( std::string("HIP error: ") + hipGetErrorString( e_) + " in " #EXPR); } while (0)

inline std::atomic<unsigned long long>& allocFailureThreshold() { static std::atomic<unsigned long long> v( 0); return v; }

struct DeviceBuffer
{
	void* ptr;
	size_t bytes;
	DeviceBuffer() :ptr(0),bytes(0){}
	~DeviceBuffer() { release(); }
	void release() { if (ptr) { (void)hipFree( ptr); ptr = 0; bytes = 0; } }
	// exact (re)allocation
	void alloc( size_t n)
	{
		release();
		if (n == 0) n = 16;
		// test hook (sp_test_fail_alloc_above, tests/test_l2_gpu.py): allocations of at least this many bytes fail like an
		// out-of-memory hipMalloc; 0 = off.  Set through the C-ABI only: nothing on the allocation path reads the environment.
		const unsigned long long failAbove = allocFailureThreshold().load( std::memory_order_relaxed);
		if (failAbove && n >= failAbove) throw HipError( "HIP error: out of memory (injected by sp_test_fail_alloc_above) in hipMalloc");
		HIP_CHECK( hipMalloc( &ptr, n));
		bytes = n;
	}
	// grow-only
	void reserve( size_t n)
	{
		if (n > bytes) alloc( n + n/4);
	}
	void upload( const void* src, size_t n)
	{
		alloc( n);
		if (n) HIP_CHECK( hipMemcpy( ptr, src, n, hipMemcpyHostToDevice));
	}
private:
	DeviceBuffer( const DeviceBuffer&);
	void operator=( const DeviceBuffer&);
};

// A buffer of `count` elements.  The count follows the buffer: a failed allocation leaves {NULL, 0}, never {NULL, old count}.
struct CountedBuffer
{
	DeviceBuffer buf;
	uint64_t count = 0;
	void* ptr() const { return buf.ptr; }
	// exact reallocation for n elements
	void realloc( uint64_t n, size_t elemBytes) { count = 0; buf.alloc( (size_t)n * elemBytes); count = n; }
	// grow-only
	void ensure( uint64_t n, size_t elemBytes) { if (count < n) realloc( n, elemBytes); }
};

// A stream of the context's own (non-blocking), created on demand; synchronised, then destroyed with its owner.
struct Stream
{
	hipStream_t h = 0;
	int device = 0;
	Stream() = default;
	Stream( const Stream&) = delete;
	~Stream() { if (h) { (void)hipSetDevice( device); (void)hipStreamSynchronize( h); (void)hipStreamDestroy( h); } }
	void create( int device_) { if (!h) { device = device_; HIP_CHECK( hipStreamCreateWithFlags( &h, hipStreamNonBlocking)); } }
	operator hipStream_t() const { return h; }
};

struct Event
{
	hipEvent_t h = 0;
	Event() = default;
	Event( const Event&) = delete;
	~Event() { if (h) (void)hipEventDestroy( h); }
	void create() { if (!h) HIP_CHECK( hipEventCreate( &h)); }
	operator hipEvent_t() const { return h; }
};

// milliseconds between two recorded events that have completed
inline bool elapsedMs( hipEvent_t from, hipEvent_t to, double& ms)
{
	float f = 0.0f;
	if (hipEventElapsedTime( &f, from, to) != hipSuccess) return false;
	ms = (double)f;
	return true;
}

// a copy on `stream`, complete when the call returns
inline void copySync( hipStream_t stream, void* dst, const void* src, size_t n, hipMemcpyKind kind)
{
	HIP_CHECK( hipMemcpyAsync( dst, src, n, kind, stream));
	HIP_CHECK( hipStreamSynchronize( stream));
}

} // namespace
#endif
