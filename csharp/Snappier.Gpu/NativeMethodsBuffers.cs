// P/Invoke surface of libsnappier_hip_buffers.so -- one declaration per function of include/snappier_hip_buffers.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsBuffers
{
    private const string Lib = "snappier_hip_buffers";                          // libsnappier_hip_buffers.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): buffers of any length, one Snappy block each
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_compress_buffers_workspace(uint nbuffers, uint maxFragments);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_compress_buffers_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nbuffers, uint maxFragments, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
