// P/Invoke surface of libsnappier_hip_frame_buffers.so -- one declaration per function of include/snappier_hip_frame_buffers.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameBuffers
{
    private const string Lib = "snappier_hip_frame_buffers";                    // libsnappier_hip_frame_buffers.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): many framed streams per call
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_encode_buffers_workspace(uint nbuffers, uint maxChunks);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_encode_buffers_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nbuffers, uint maxChunks, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_decode_buffers_workspace(uint nstreams, uint maxChunks, uint maxSpans);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_decode_buffers_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, uint maxChunks, uint maxSpans, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
