// P/Invoke surface of libsnappier_hip_frame_range.so -- one declaration per function of include/snappier_hip_frame_range.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameRange
{
    private const string Lib = "snappier_hip_frame_range";                      // libsnappier_hip_frame_range.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): a window of decoded bytes out of every framed stream
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_decode_range_workspace(uint nstreams, uint maxChunks, uint maxSpans, ulong edgeCap);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_decode_range_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dRangeOff, IntPtr dRangeLen, uint maxChunks, uint maxSpans, ulong edgeCap, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
