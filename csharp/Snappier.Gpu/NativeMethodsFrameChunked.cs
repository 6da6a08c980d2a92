// P/Invoke surface of libsnappier_hip_frame_chunked.so -- one declaration per function of include/snappier_hip_frame_chunked.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameChunked
{
    private const string Lib = "snappier_hip_frame_chunked";                    // libsnappier_hip_frame_chunked.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): framed streams with a chosen chunk size, and their seek index
    // (the five dIdx* pointers are all IntPtr.Zero for "no index", else all given: the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_encode_chunked_workspace(uint nbuffers, uint maxChunks, uint chunkBytes);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_encode_chunked_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nbuffers, uint chunkBytes, uint maxChunks, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, IntPtr dWork, IntPtr dResult);
}
