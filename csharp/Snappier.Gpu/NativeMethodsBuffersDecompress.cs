// P/Invoke surface of libsnappier_hip_buffers_decompress.so -- one declaration per function of include/snappier_hip_buffers_decompress.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsBuffersDecompress
{
    private const string Lib = "snappier_hip_buffers_decompress";               // libsnappier_hip_buffers_decompress.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): snp_decompress_batch that splits large blocks across wavefronts
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_decompress_buffers_workspace(uint nbuffers, uint maxFragments);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_decompress_buffers_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nbuffers, uint maxFragments, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dWork, IntPtr dResult);
}
